/*
 * ttsdec.h - C ABI of libttsdec.so: the MI355X (gfx950) implementation of the
 * Tacotron autoregressive mel-decoder hot path of kgoba/torch-tts.
 *
 * The reference has no FFI / plugin interface for this path: its boundary is the
 * Python module API (tacotron/decoder.py:6-18 Decoder, tacotron/decoder_cell.py:143-195
 * Taco2ProdDecoderCell, tacotron/modules/modules.py:155-184 MelPostnet).  This C ABI is
 * what the host-side mirror of those modules (the Python files of torch-tts_amd/, ctypes) binds; each
 * entry point below names the reference code it replaces.  INTEGRATION.md shows the
 * reference-side stub.
 *
 * Conventions
 *   - plain pointers and sizes only; every data pointer is a DEVICE pointer (fp32,
 *     row-major contiguous) unless it says "host".
 *   - the caller owns every buffer (weights blob, workspace, inputs, outputs); the
 *     library allocates nothing on the device and keeps only the pointers bound with
 *     ttsdec_bind_weights().
 *   - all work is enqueued on the hipStream_t passed in (as void*); nothing on the decode / postnet / encoder / VITS2 paths
 *     synchronises.  The two exceptions are set-up calls and say so below: ttsdec_pack_weights (one stream synchronisation +
 *     an 8-byte read-back for the range guard) and ttsdec_bind_weights (a synchronous 8-byte copy of the same header).
 *     Calls on one handle must be serialised by the caller.
 *   - return value: 0 = TTSDEC_OK, negative = error (ttsdec_strerror()).  Nothing
 *     throws or aborts across this boundary.
 *   - the handle is bound to the HIP device that was current at ttsdec_create();
 *     that device must be current for every later call.
 */
#ifndef TTSDEC_H
#define TTSDEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version: bumped whenever an entry point's argument list or a struct layout changes.  2 (round 4): ttsenc_forward /
 * ttsvits_text_encoder / ttsvits_flow_reverse carry `g` and a status word, ttsvits_dims two more fields (round 3, unversioned
 * then); ttsenc_set_precision / ttsenc_get_precision added, and exact fp32 became the default arithmetic of the ttsenc_ / ttsvits_
 * handles as it always was of the ttsdec_ ones (split-fp16 is opt-in everywhere).  The Python binding refuses a library whose ttsdec_version() differs from the version it was written for. */
#define TTSDEC_VERSION 2
/* (The ttsgen_ family below - the HiFi-GAN generator - was added later without a bump: it adds entry points and a struct of its
 * own and changes none that existed, so a version-2 binding still binds every entry point it knows.) */
/* (So was the ttsdur_ family at the end - the duration predictors and the length regulator - for the same reason.) */
/* (And ttsvits_flow_forward and the ttspost_ family - the posterior encoder - for voice conversion; then ttsvits_neg_cent,
 * ttsvits_maximum_path and ttsvits_align for monotonic alignment search; then ttsvits_spectrogram, ttsvits_spec_to_mel and
 * ttsvits_mel_spectrogram, the spectrogram front-end; then ttsdec_griffinlim_workspace_bytes, ttsdec_mel_to_magnitude and
 * ttsdec_griffinlim, mel -> waveform for the Tacotron path; then ttsdec_mel_analysis_workspace_bytes and ttsdec_mel_analysis,
 * waveform -> dB spectrogram and mel for it; then ttsvits_generator_planes_bytes, _pack_planes, _workspace_bytes and _forward,
 * the generator with its arithmetic as a call argument; then ttsdec_resample_workspace_bytes and ttsdec_resample, sample-rate
 * conversion in front of ttsdec_mel_analysis; then ttsvits_disc_*, the waveform discriminators, a second handle kind under
 * ttsvits_ with a struct of its own; then ttsvits_durdisc_*, the duration discriminators, a third one; then ttsvits_durnll_*, the
 * stochastic duration predictor's likelihood, a fourth; then ttsvits_kl_loss_workspace_bytes, ttsvits_kl_loss,
 * ttsvits_slice_segments and ttsvits_sliced_l1, the glue of the validation step; then ttsdec_val_losses_workspace_bytes,
 * ttsdec_val_losses and ttsdec_mel_loss, the loss terms of the Tacotron validation step.) */

enum {
  TTSDEC_OK = 0,
  TTSDEC_ERR_INVALID_ARG = -1, /* null pointer, negative size, bad enum */
  TTSDEC_ERR_DIMS = -2,        /* a feature dimension is not a multiple of 4 / out of range */
  TTSDEC_ERR_HIP = -3,         /* a HIP runtime call failed (hipGetLastError text via ttsdec_last_hip_error) */
  TTSDEC_ERR_NOT_BOUND = -4,   /* decode/postnet before ttsdec_bind_weights */
  TTSDEC_ERR_WORKSPACE = -5,   /* workspace too small or misaligned */
  TTSDEC_ERR_DEVICE = -6       /* current device differs from the handle's, or is not gfx950 */
};

/* Model dimensions.  Source of truth: configs/config-ljspeech.yaml:47-69 via
 * build_tacotron (tacotron/tacotron.py:165-214). */
typedef struct ttsdec_dims {
  int32_t d_mel;           /* audio.num_mels                     (80)   */
  int32_t r;               /* decoder.r, frames per step          (1)   */
  int32_t d_pre;           /* decoder.dim_pre, both PreNet layers (256) */
  int32_t d_ctx;           /* encoder.dim_out                     (512) */
  int32_t h_att;           /* decoder.dim_rnn[0]                  (1024)*/
  int32_t h_dec;           /* decoder.dim_rnn[1]                  (1024)*/
  float p_zoneout;         /* decoder_cell.py:145                 (0.1) */
  float p_dropout;         /* modules.py:25 PreNet p_dropout      (0.5) */
  int32_t postnet_layers;  /* model.postnet.num_layers            (3); 0 = no postnet */
  int32_t postnet_hidden;  /* model.postnet.dim_hidden            (512) */
  int32_t postnet_kernel;  /* MelPostnet kernel_size              (5)   */
  float bn_eps;            /* nn.BatchNorm1d eps                  (1e-5)*/
  int32_t cell_type;       /* TTSDEC_CELL_*: which decoder cell of decoder_cell.py                  */
  int32_t d_pre_hidden;    /* width of PreNet layer 0; 0 = d_pre (Taco2ProdDecoderCell, decoder_cell.py:152);
                            * Taco2DecoderCell uses 128 (decoder_cell.py:74-76)                      */
  int32_t postnet_type;    /* TTSDEC_POSTNET_TYPE_*                                                  */
} ttsdec_dims;

/* Decoder cells (tacotron/tacotron.py:171-176 picks by model.decoder.type). */
enum {
  TTSDEC_CELL_TACO2PROD = 0, /* Taco2ProdDecoderCell (decoder_cell.py:143-195): LJSpeech config.  h_att / h_dec are the
                              * attention-rnn and decoder-rnn widths.                                               */
  TTSDEC_CELL_TACO2 = 1      /* Taco2DecoderCell (decoder_cell.py:66-140): rdh / sandra / template configs.  Context from
                              * the previous weights feeds both stacked LSTMs (h_att = dim_rnn[0], h_dec = dim_rnn[1]);
                              * query and projection read cat[h0, h1, zeros]; no ctx in the state.                   */
};
/* Postnets (tacotron/tacotron.py:199-214 picks by model.postnet.type). */
enum {
  TTSDEC_POSTNET_TYPE_MEL = 0,  /* MelPostnet  (modules/modules.py:155-184)                                            */
  TTSDEC_POSTNET_TYPE_MEL2 = 1  /* MelPostnet2 (modules/modules.py:187-216): postnet_layers residual blocks of
                                 * Conv1dFix-BN-LeakyReLU x2 + Conv1dFix (mps_fixes.py:6-29)                           */
};

typedef struct ttsdec_handle ttsdec_handle;

/* Order of the source tensors handed to ttsdec_pack_weights: the reference's
 * state-dict order.  Postnet entries repeat per layer. */
enum {
  TTSDEC_W_PRE0_W = 0, /* decoder.decoder_cell.pre_net.layers.0.weight [d_pre_hidden, d_mel] */
  TTSDEC_W_PRE0_B,     /* ...layers.0.bias   [d_pre_hidden]                                   */
  TTSDEC_W_PRE1_W,     /* ...layers.1.weight [d_pre, d_pre_hidden]                            */
  TTSDEC_W_PRE1_B,     /* ...layers.1.bias   [d_pre]                                          */
  TTSDEC_W_QUERY_W,    /* decoder_cell.attention_module.query_layer.weight [d_ctx, h_att]     */
  TTSDEC_W_ATT_IH,     /* decoder_cell.attention_rnn.weight_ih [4*h_att, d_pre+d_ctx]         */
  TTSDEC_W_ATT_HH,     /* ...weight_hh [4*h_att, h_att]                                       */
  TTSDEC_W_ATT_BIH,    /* ...bias_ih   [4*h_att]                                              */
  TTSDEC_W_ATT_BHH,    /* ...bias_hh   [4*h_att]                                              */
  TTSDEC_W_DEC_IH,     /* decoder_cell.decoder_rnn.weight_ih [4*h_dec, h_att+d_ctx]           */
  TTSDEC_W_DEC_HH,     /* ...weight_hh [4*h_dec, h_dec]                                       */
  TTSDEC_W_DEC_BIH,    /* ...bias_ih   [4*h_dec]                                              */
  TTSDEC_W_DEC_BHH,    /* ...bias_hh   [4*h_dec]                                              */
  TTSDEC_W_INIT_H0,    /* decoder_cell.initial_decoder_h.0 [1, h_att]                         */
  TTSDEC_W_INIT_H1,    /* decoder_cell.initial_decoder_h.1 [1, h_dec]                         */
  TTSDEC_W_INIT_C0,    /* decoder_cell.initial_decoder_c.0 [1, h_att]                         */
  TTSDEC_W_INIT_C1,    /* decoder_cell.initial_decoder_c.1 [1, h_dec]                         */
  TTSDEC_W_MEL_W,      /* decoder.fc_mel.weight  [r*d_mel, h_dec+d_ctx]                       */
  TTSDEC_W_MEL_B,      /* decoder.fc_mel.bias    [r*d_mel]                                    */
  TTSDEC_W_STOP_W,     /* decoder.fc_stop.weight [r, h_dec+d_ctx]                             */
  TTSDEC_W_STOP_B,     /* decoder.fc_stop.bias   [r]                                          */
  /* TTSDEC_CELL_TACO2 uses the same slots: QUERY_W is [d_ctx, h_att+h_dec+d_ctx]; ATT_* / DEC_* are
   * decoder_rnn_list.0 / .1 ([4*h_att, d_pre+d_ctx], [4*h_dec, h_att+d_ctx]); MEL_W / STOP_W have
   * h_att+h_dec+d_ctx columns. */
  TTSDEC_W_DECODER_COUNT, /* = 21; postnet tensors follow:                                   */
  /* per layer i (5 each): postnet.conv.i.0.weight [C_out, C_in, k], conv.i.1.weight [C_out],
   * conv.i.1.bias, conv.i.1.running_mean, conv.i.1.running_var; then postnet.fc_out.weight
   * [d_mel, hidden].  Total = 21 + 5*postnet_layers + 1 (or 21 when postnet_layers == 0). */
  TTSDEC_W_POSTNET_PER_LAYER = 5,
  /* TTSDEC_POSTNET_TYPE_MEL2, per layer i (11 each, no fc_out): postnet.layers.i.1.weight [hidden, d_mel, k],
   * layers.i.2.{weight,bias,running_mean,running_var}, layers.i.5.weight [hidden, hidden, k],
   * layers.i.6.{weight,bias,running_mean,running_var}, layers.i.9.weight [d_mel, hidden, k]. */
  TTSDEC_W_POSTNET2_PER_LAYER = 11
};

/* Prenet dropout modes (the reference's dropout is always on, modules.py:40). */
enum {
  TTSDEC_DROPOUT_OFF = 0,   /* no dropout (not reference behaviour; for analysis)              */
  TTSDEC_DROPOUT_MASKS = 1, /* keep-masks injected: uint8 [steps, 2, B, d_pre], 1 = keep       */
  TTSDEC_DROPOUT_PHILOX = 2 /* on-device Philox4x32-10 keyed by (seed; step, layer, b, unit): one keep BIT per
                             * unit, i.e. keep probability exactly 1/2 - valid only for p_dropout == 0.5 (the
                             * reference's value, modules.py:25); other p: TTSDEC_ERR_INVALID_ARG, use MASKS   */
};

/* Arithmetic of the step's GEMMs: the two LSTM gate GEMMs (95 % of the step's FLOPs), the PreNet, the query and the
 * mel/stop projection. */
enum {
  TTSDEC_PREC_F32 = 0,       /* exact fp32 on the fp32-input matrix instruction (default)             */
  TTSDEC_PREC_SPLIT_F16 = 1  /* split-fp16: x = hi + lo*2^-11 (two fp16 planes, 22 significand bits),
                              * a*b = ah*bh + (ah*bl + al*bh)*2^-11 on the f16 matrix instruction with
                              * fp32 accumulation; ~2^-22 relative per product.  Needs d_pre, d_ctx,
                              * h_att, h_dec to be multiples of 8, else the handle stays on F32.      */
};

/* Postnet arithmetic. */
enum {
  TTSDEC_POSTNET_F32 = 0,       /* exact fp32 (fp32-input MFMA)                                              */
  TTSDEC_POSTNET_BF16 = 1,      /* bf16 operands on the bf16 MFMA, fp32 accumulate (BASELINE.json configs[2]):
                                 * ~3 significant digits; the tolerance is reported by the tests/bench       */
  TTSDEC_POSTNET_SPLIT_F16 = 2  /* split-fp16 operands (see TTSDEC_PREC_SPLIT_F16): fp32-grade               */
};                              /* 16-bit modes need d_mel and postnet_hidden to be multiples of 8, else F32 is used */

int ttsdec_version(void);
const char* ttsdec_strerror(int code);
/* Text of the last HIP error seen on this handle ("" if none).  Host string, owned by the library. */
const char* ttsdec_last_hip_error(const ttsdec_handle* h);

/* Replaces: module construction in build_tacotron (tacotron/tacotron.py:178-206). */
int ttsdec_create(const ttsdec_dims* dims, ttsdec_handle** out);
int ttsdec_destroy(ttsdec_handle* h);

/* Selects TTSDEC_PREC_* for later decode / cell_step calls (weights of both forms live in
 * the packed blob, so this can be switched at any time).  ttsdec_get_precision returns the
 * mode actually in effect for the handle's dims. */
int ttsdec_set_precision(ttsdec_handle* h, int precision);
int ttsdec_get_precision(const ttsdec_handle* h);

/* Tuning and measurement options of a decoder handle.  The defaults (value -1) are the measured-best settings per batch size
 * and arithmetic mode; nothing here changes results beyond the summation order of a GEMM's K segments (every setting is
 * held to the same parity bar by tests/test_hip_parity.py::test_all_step_orders_and_layouts_vs_oracle).  Setting an
 * option drops the handle's captured graph.  MEASUREMENT ONLY - not part of the drop-in surface.
 * The environment variable TTSDEC_OPTIONS="name=value,name=value" (names below, lower case without the prefix) presets
 * the options of every handle created afterwards; it is read once per ttsdec_create.  The only other environment
 * variables the library reads, all measurement-only as well: TTSDEC_STAMPS=<file> (per-workgroup time stamps of the
 * two-role launches of a decode call's last step, written to <file>; synchronises the stream),
 * TTSDEC_NO_LEAN_SKINNY=1 (short-K row GEMMs of the VITS2 path back on the 128 x 128 tile), TTSDEC_LEAN8_F32_MAX=<rows>
 * (largest batch on the 32-row exact-fp32 LSTM tile), TTSDEC_CONV256=0 (the Postnet's hidden conv layers back on the
 * shared GEMM tile) and TTSDEC_CONV256_FORCE=1 (those layers on the 256 x 256 kernel even where its tiles do not fill
 * the chip - the tests' switch). */
enum {
  TTSDEC_OPT_GRAPH = 0,        /* "graph": 0 = launch every step kernel from the host instead of replaying a captured hipGraph  */
  TTSDEC_OPT_OVERLAP,          /* "overlap": two-role launches 0 = none, 1 = frame || lstm_att, 2 = also attention || lstm_dec;
                                * a larger value means 2                                                                      */
  TTSDEC_OPT_CHUNK_A,          /* "chunk_a": 0 = row-major fp16 activation planes instead of the chunked layout                */
  TTSDEC_OPT_CHUNK_B,          /* "chunk_b": 0 = row-major LSTM weight planes                                                  */
  TTSDEC_OPT_PROJ_REGW,        /* "proj_regw": 0 = mel/stop projection on the LDS-staged split-K GEMM                          */
  TTSDEC_OPT_HEAD_PROJ,        /* "head_proj": 1 / 0 = that projection as a role at the head of the next step's first launch   */
  TTSDEC_OPT_QUERY_ROLE,       /* "query_role": 1 / 0 = the attention query GEMM as a job of the attention role's workgroups
                                * (overlap 2, at most 512 utterances) instead of a launch of its own                          */
  TTSDEC_OPT_ATTN_FORM,        /* "attn_form": measurement. The form of the attention pass beside the exact-fp32 decoder LSTM on
                                * the 64 x 16 tile: <= 0 = the regime default (lean), 1 = base, 2 = one row (ablation),
                                * 3 = plain sum (ablation), 4 = base with swapped wave priorities, 5 = lean                   */
  TTSDEC_OPT_PROFILE_ABLATION, /* "profile_ablation": ttsdec_profile_step only, kernel-internal ablation switches              */
  TTSDEC_OPT_DEBUG_FLAGS,      /* "debug_flags": TEST HOOK. bit 0 / 1 / 2: the frame / attention / projection-head role of a
                                * two-role launch does not signal its consumers, which then run into the bounded-spin
                                * time-out (T_out[1] bit 2)                                                                   */
  TTSDEC_OPT_SPIN_LIMIT,       /* "spin_limit": TEST HOOK. polls before a consumer role gives up (default 4096, ~1-4 ms)         */
  TTSDEC_OPT_COUNT
};
int ttsdec_set_option(ttsdec_handle* h, int option, int value);
int ttsdec_get_option(const ttsdec_handle* h, int option, int* value);
const char* ttsdec_option_name(int option); /* NULL for an unknown option */

/* Number of source tensors ttsdec_pack_weights expects for these dims. */
int ttsdec_num_weight_tensors(const ttsdec_handle* h);
/* Size of the packed weight blob (bytes, multiple of 256). */
size_t ttsdec_packed_bytes(const ttsdec_handle* h);

/* Packs the reference-layout parameters into the kernel layout inside `blob`
 * (caller-allocated, ttsdec_packed_bytes(), 256-B aligned): sums the LSTM bias
 * pairs, stacks fc_mel/fc_stop, transposes conv weights to [C_out][tap][C_in],
 * turns BatchNorm running stats into per-channel (alpha, beta).  The blob is
 * position-independent: it can be broadcast to other GPUs (RCCL) and bound there.
 * Range guard of the split-fp16 planes: the call also reduces max |w| over the matrices that have
 * planes into the blob header and reads it back - the ONE place this library synchronises `stream`.
 * A weight with |w| >= 65504 (or NaN) has no split-fp16 form: the handle then stays on exact fp32
 * for the affected GEMMs whatever ttsdec_set_precision / the postnet precision ask
 * (ttsdec_get_precision reports the mode in effect).
 * Replaces: nn.Module parameter storage / load_state_dict (train_util.py:23-45). */
int ttsdec_pack_weights(ttsdec_handle* h, const float* const* src /*host array of device ptrs; NULL entry = skip*/, int n_src,
                        void* blob, void* stream);
/* Binds a packed blob (from ttsdec_pack_weights here or on another rank).  The blob must be complete
 * (e.g. the broadcast that fills it finished): its header (the range guard's maxima) is read back here
 * with a synchronous copy. */
int ttsdec_bind_weights(ttsdec_handle* h, const void* blob);

/* Decoder workspace (recurrent state + scratch) for a batch of B utterances with
 * memory length L.  The state persists in the workspace between ttsdec_decode calls.
 * Size limit (also ttsenc_workspace_bytes and ttsenc_style_workspace_bytes): the LSTM kernels reach their operands through one
 * buffer descriptor of 0x7FFFF000 bytes (just under 2 GiB), so a (B, L) whose workspace would be that large or larger is refused
 * - the query returns 0 and the calls that take the workspace return TTSDEC_ERR_WORKSPACE - and a handle whose packed blob
 * would be (ttsdec_create, ttsenc_create, ttsenc_style_create) is refused with TTSDEC_ERR_DIMS.  It takes a batch in the
 * ten-thousands to get there. */
size_t ttsdec_workspace_bytes(const ttsdec_handle* h, int B, int L);

/*
 * Runs decode steps t_begin .. t_begin+n_steps-1 of Decoder.forward
 * (tacotron/decoder.py:47-71) for the whole batch; one step = PreNet ->
 * attention LSTM -> stepwise-monotonic attention -> context -> decoder LSTM ->
 * mel/stop projection (tacotron/decoder_cell.py:180-195).
 *
 *   memory        [B, L, d_ctx] encoder outputs (zero on padded rows)
 *   t_begin       global index of the first step of this call (must be even); 0 (re)initialises
 *                 the recurrent state from the initial_decoder_{h,c} parameters
 *                 (decoder_cell.py:165-178) and the GO frame (decoder.py:35)
 *   n_steps       steps to run at most in this call
 *   t_stride      capacity (in steps) of the output buffers of this call, >= n_steps
 *   stop_threshold / check_stop
 *                 inference stop rule (decoder.py:68): the first step at which ANY
 *                 utterance's stop logit < threshold is the last one produced
 *                 (inclusive, batch-global); later steps of this and following
 *                 calls are skipped.  check_stop = 0 disables it (teacher mode).
 *   dropout_mode  TTSDEC_DROPOUT_*; masks for MASKS: per step (relative to t_begin) the keep-mask
 *                 of PreNet layer 0 [B, d_pre_hidden] followed by layer 1 [B, d_pre], uint8
 *                 (= [n_steps, 2, B, d_pre] when the two widths are equal); seed for PHILOX
 *   teacher       optional [B, teacher_T, d_mel] ground-truth frames (decoder.py:38-42);
 *   teacher_flags optional uint8 [>= t_begin+n_steps]: flags[t-1] != 0 => the input of
 *                 step t (t >= 1) is teacher frame t*r-1 instead of the model's own
 *                 last frame (decoder.py:65-66).  NULL teacher = free-running.
 *   y [B, t_stride*r, d_mel], s [B, t_stride*r], w [B, t_stride, L]
 *                 outputs of this call, step t stored at row (t - t_begin)
 *   T_out         device int32[2]: [0] = total number of steps produced so far
 *                 (= stop step + 1 if the rule fired, else t_begin+n_steps),
 *                 [1] = bit 0: the stop rule has fired; bit 2: a two-role launch of the step gave up waiting
 *                 for its producer role (bounded spin of ~1-4 ms, once per call: later gates of the same call
 *                 return at once; only possible when the producer role's workgroups are not resident - a GPU
 *                 shared with another process's kernels, a stalled queue): the outputs of the call are INVALID.
 *                 What a direct caller of this ABI must do then (torch-tts_amd/decoder.py does exactly this):
 *                 ttsdec_set_option(h, TTSDEC_OPT_OVERLAP, 0) and ttsdec_set_option(h, TTSDEC_OPT_HEAD_PROJ, 0) -
 *                 one role per launch, no hand-off inside a launch - and decode the utterance batch again from
 *                 t_begin = 0 (the recurrent state left in the workspace is not a state of the sequence any more);
 *                 bit 1 (split-fp16 mode only): an activation
 *                 entering a 16-bit GEMM (input / teacher frame, PreNet output, context) had
 *                 |x| > 65504, the fp16 range - it was SATURATED, never inf/NaN, so outputs stay
 *                 finite but those rows are not fp32-accurate: rerun with TTSDEC_PREC_F32.
 *                 (Activation bound of the split mode: |x| <= 65504; h is bounded by 1, the context
 *                 by max |memory|.)
 *   State after a fired stop: the outputs up to and including the stop step are final, but the recurrent state left in the
 *   workspace is NOT the state at the stop step (launches that overlap the next step's early work have already advanced
 *   parts of it: the attention LSTM's cell state is one step past the stop frame).  A decode that stopped cannot be
 *   continued; start the next utterance batch with t_begin = 0.
 */
int ttsdec_decode(ttsdec_handle* h, const float* memory, int B, int L, int t_begin, int n_steps, int t_stride,
                  float stop_threshold, int check_stop, int dropout_mode, const uint8_t* masks, uint64_t seed,
                  const float* teacher, int teacher_T, const uint8_t* teacher_flags, float* y, float* s, float* w,
                  int32_t* T_out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * ttsdec_decode, free-running, under the PER-UTTERANCE stop rule (batched synthesis): every argument ttsdec_decode takes but
 * check_stop, and
 *
 *   stop_steps    device int32 [B].  Utterance b STOPS at the first step t_b at which any of its r stop logits is
 *                 < stop_threshold; stop_steps[b] = t_b then, and later crossings of the same utterance change nothing.  An
 *                 utterance that has not fired holds 0x7fffffff.  A call with t_begin = 0 resets the array (and the count of
 *                 stopped utterances, which lives in the workspace) together with the recurrent state; calls with t_begin > 0
 *                 continue it, so the chunks of one decode must pass the same array.
 *   The CALL fires at t_all = max_b t_b, the step at which the last live utterance stops: from there on everything is as
 *   after the batch-global rule fired at t_all - the outputs are final through step t_all inclusive, later steps of this and
 *   following calls are skipped, the "State after a fired stop" note above applies.
 *   An utterance that has stopped is still computed up to t_all (the tiles are fixed): its outputs at steps > t_b are
 *   don't-care; ttsdec_zero_tail clears them.
 *   T_out         [0] = t_all + 1 if the call has fired, else t_begin + n_steps; [1]: the flag bits of ttsdec_decode.  Bit 1,
 *                 the split-fp16 range flag, may also be raised by an utterance past its own stop step, whose free-running
 *                 frames nobody bounds.
 *   teacher       must be NULL (TTSDEC_ERR_INVALID_ARG otherwise, as for stop_steps == NULL and an odd t_begin): the
 *                 per-utterance rule is free-running only.  teacher_T and teacher_flags are ignored.
 * For B = 1 this is ttsdec_decode with check_stop = 1, bit for bit; for any B the arithmetic of a step is ttsdec_decode's.
 */
int ttsdec_decode_each(ttsdec_handle* h, const float* memory, int B, int L, int t_begin, int n_steps, int t_stride,
                       float stop_threshold, int dropout_mode, const uint8_t* masks, uint64_t seed, const float* teacher,
                       int teacher_T, const uint8_t* teacher_flags, float* y, float* s, float* w, int32_t* stop_steps,
                       int32_t* T_out, void* workspace, size_t workspace_bytes, void* stream);

/* Zeroes rows [lengths[b] / len_div, T) of every entry b of x [B, T, C] fp32, entries batch_stride floats apart (>= T * C): what
 * a ragged batch holds past each utterance's end.  lengths: device int32 [B], clamped to [0, T * len_div]; B <= 65535.  Write-only,
 * and only over the padding.  (After ttsdec_decode_each: y with C = d_mel, s with C = 1, w with C = L, T in steps and
 * len_div = r for lengths in frames.) */
int ttsdec_zero_tail(ttsdec_handle* h, float* x, const int32_t* lengths, int B, int T, int64_t batch_stride, int C, int len_div,
                     void* stream);

/* Postnet scratch for B*T frames. */
size_t ttsdec_postnet_workspace_bytes(const ttsdec_handle* h, int B, int T);

/* MelPostnet.forward in eval mode (tacotron/modules/modules.py:178-184):
 * y [B, T, d_mel] -> y_post [B, T, d_mel] = y + fc_out(isru(BN(conv(...)))); or, for
 * TTSDEC_POSTNET_TYPE_MEL2, MelPostnet2.forward (modules.py:213-216). */
int ttsdec_postnet(ttsdec_handle* h, const float* y, int B, int T, int precision, float* y_post, void* workspace,
                   size_t workspace_bytes, void* stream);

/* The Postnet on a ragged batch: row b of y_post, frames [0, lengths[b]), is what ttsdec_postnet gives for y[b, :lengths[b]]
 * alone (B = 1, T = lengths[b]) - the input of every conv layer, y and each hidden activation, is zero at frames
 * >= lengths[b], and so is y_post.  What y holds there is never used.
 *   lengths       device int32 [B], frames, each in [0, T] (0: an all-zero row; values outside are clamped); B <= 65535.
 *                 NULL = ttsdec_postnet: the same launches, the same bits.
 * Same workspace (ttsdec_postnet_workspace_bytes).  The conv kernels are ttsdec_postnet's; between them a write-only pass zeroes
 * each activation's padding. */
int ttsdec_postnet_ragged(ttsdec_handle* h, const float* y, const int32_t* lengths, int B, int T, int precision, float* y_post,
                          void* workspace, size_t workspace_bytes, void* stream);

/* One decoder-cell step on caller-held state (Taco2ProdDecoderCell.forward,
 * tacotron/decoder_cell.py:180-195), for callers that drive the cell directly.
 * Not needed by Decoder.forward; provided for API completeness.  State tensors are
 * updated in place: w [B,L], ctx [B,d_ctx], h_att/c_att [B,h_att], h_dec/c_dec [B,h_dec];
 * x [B, d_mel] is the input frame; x_dec [B, h_dec+d_ctx] receives cat[h_dec, ctx].
 * TTSDEC_CELL_TACO2 (decoder_cell.py:110-140): ctx is output only (the context the LSTMs consumed,
 * = bmm(w_in, memory)); x_dec is [B, h_att+h_dec+d_ctx] = cat[h0, h1, zeros].
 * masks: [2, B, d_pre] uint8 or NULL per dropout_mode; step only keys the Philox stream. */
int ttsdec_cell_step(ttsdec_handle* h, const float* x, const float* memory, int B, int L, float* w, float* ctx,
                     float* h_att, float* c_att, float* h_dec, float* c_dec, int dropout_mode, const uint8_t* masks,
                     uint64_t seed, int step, float* x_dec, void* workspace, size_t workspace_bytes, void* stream);

/* Measurement aid for bench.py: runs `iters` decode steps on the current
 * workspace state and reports the mean duration (ms, HIP events on `stream`) of each
 * kernel of the step, in launch order, into ms_out[0..n_out) (host array); returns the
 * number of kernels per step in *n_kernels and their names (static strings) in names_out.
 * The profiled step is step 1 of a two-step call: y [B, 2r, d_mel], s [B, 2r], w [B, 2, L]. */
int ttsdec_profile_step(ttsdec_handle* h, const float* memory, int B, int L, int iters, int dropout_mode,
                        const uint8_t* masks, uint64_t seed, float* y, float* s, float* w, void* workspace,
                        size_t workspace_bytes, void* stream, float* ms_out, const char** names_out, int n_out,
                        int* n_kernels);

/* Measurement aid for bench.py: the step's launches timed INSIDE the replayed graph of the step loop.  Runs one ordinary
 * decode call of n_steps steps from step 0 (a multiple of the graph's 30 steps, >= 60; stop rule off) in which workgroup 0 of
 * every step kernel stores its start time (one 8-byte store per launch: the only difference to ttsdec_decode); ms_out[k] is
 * the mean time from launch k's start to the next launch's start - the launch's duration in the loop including the gap
 * behind it - over the last graph replay; the entries add up to *step_ms, the loop's time per step.  Synchronises the
 * stream.  Names and counts as for ttsdec_profile_step; y [B, n_steps*r, d_mel], s [B, n_steps*r], w [B, n_steps, L]. */
int ttsdec_profile_loop(ttsdec_handle* h, const float* memory, int B, int L, int n_steps, int dropout_mode, const uint8_t* masks,
                        uint64_t seed, float* y, float* s, float* w, int32_t* T_out, void* workspace, size_t workspace_bytes, void* stream,
                        float* ms_out, const char** names_out, int n_out, int* n_kernels, float* step_ms);

/* ---------------------------------------------------------------------------------------
 * Text encoder: Encoder2.forward in eval mode, tacotron/encoder.py:27-82
 * with the packed bidirectional LSTM of tacotron/modules/rnn.py:112-127.  Produces the `memory`
 * the decoder consumes.  Runs once per batch; split-fp16 GEMMs for the convs and the input projection (fp32-class accuracy), exact fp32 recurrence.
 * ------------------------------------------------------------------------------------- */
typedef struct ttsenc_dims {
  int32_t alphabet_size; /* 1 + len(text.alphabet) (+ phonemes), tacotron.py:189-191 */
  int32_t d_emb;         /* model.encoder.dim_emb (512): embedding and conv channels  */
  int32_t d_out;         /* model.encoder.dim_out (512): 2 x LSTM hidden              */
  int32_t conv_kernel;   /* 5                                                          */
  float bn_eps;          /* 1e-5                                                       */
} ttsenc_dims;
typedef struct ttsenc_handle ttsenc_handle;

/* Source tensors for ttsenc_pack_weights, the reference's state-dict order below ``encoder.``. */
enum {
  TTSENC_W_EMB = 0,   /* emb.weight [alphabet, d_emb]                                   */
  TTSENC_W_CONV0,     /* conv.0.weight [d_emb, d_emb, k]                                */
  TTSENC_W_BN0_W, TTSENC_W_BN0_B, TTSENC_W_BN0_MEAN, TTSENC_W_BN0_VAR, /* conv.1.*      */
  TTSENC_W_CONV1,     /* conv.3.weight                                                  */
  TTSENC_W_BN1_W, TTSENC_W_BN1_B, TTSENC_W_BN1_MEAN, TTSENC_W_BN1_VAR, /* conv.4.*      */
  TTSENC_W_CONV2,     /* conv.6.weight                                                  */
  TTSENC_W_BN2_MEAN, TTSENC_W_BN2_VAR, /* conv.7.running_{mean,var} (affine=False)      */
  TTSENC_W_IH_FWD,    /* rnn.rnn.weight_ih_l0 [4H, 2*d_emb], H = d_out/2                */
  TTSENC_W_HH_FWD,    /* rnn.rnn.weight_hh_l0 [4H, H]                                   */
  TTSENC_W_IH_REV,    /* rnn.rnn.weight_ih_l0_reverse                                   */
  TTSENC_W_HH_REV,    /* rnn.rnn.weight_hh_l0_reverse                                   */
  TTSENC_W_H0,        /* rnn_h0 [1, 1, d_out]                                           */
  TTSENC_W_C0,        /* rnn_c0 [1, 1, d_out]                                           */
  TTSENC_W_COUNT
};

int ttsenc_create(const ttsenc_dims* dims, ttsenc_handle** out);
int ttsenc_destroy(ttsenc_handle* h);
const char* ttsenc_last_hip_error(const ttsenc_handle* h);
int ttsenc_num_weight_tensors(const ttsenc_handle* h);
size_t ttsenc_packed_bytes(const ttsenc_handle* h);
int ttsenc_pack_weights(ttsenc_handle* h, const float* const* src, int n_src, void* blob, void* stream);
int ttsenc_bind_weights(ttsenc_handle* h, const void* blob);
/* 0 for a (B, L) beyond the size limit stated at ttsdec_workspace_bytes. */
size_t ttsenc_workspace_bytes(const ttsenc_handle* h, int B, int L);
/* ids [B, L] int64 (0 = padding), lengths [B] int32 on the device; L_out = max(lengths) (host-known:
 * the reference pads its output to the longest utterance, rnn.py:126); memory [B, L_out, d_out].
 * status: optional device int32 (caller zeroes it): bit 0 is set when an id lay outside [0, alphabet_size) - nn.Embedding raises
 * IndexError there (encoder.py:69); the kernel reads the nearest table row instead of memory outside the table and the caller
 * reads the word with the results (no scan of the ids on the host, no synchronisation before the launch). */
int ttsenc_forward(ttsenc_handle* h, const int64_t* ids, const int32_t* lengths, int B, int L, int L_out, float* memory,
                   void* workspace, size_t workspace_bytes, void* stream, int32_t* status);
/* Arithmetic of the encoder's conv and input-projection GEMMs: TTSDEC_PREC_F32 (default: exact fp32, the reference's own) or
 * TTSDEC_PREC_SPLIT_F16 (two fp16 planes per operand; needs d_emb % 8 == 0, else exact fp32 stays).  The recurrence is always
 * exact fp32.  Both weight forms live in the packed blob: switchable per call. */
int ttsenc_set_precision(ttsenc_handle* h, int precision);
int ttsenc_get_precision(const ttsenc_handle* h);

/* ---------------------------------------------------------------------------------------
 * Style encoder (tacotron/modules/style.py, modules/attention.py:129-186), a second handle of the ttsenc_ family: the
 * ReferenceEncoder (n_convs x [Conv2d 3x3 stride 2 pad 1 + bias -> BatchNorm2d (running statistics) -> ReLU], then a one-layer
 * LSTM over the packed sequence, last hidden state) and what VAE / GST / GST_VAE put behind it.  Eval mode, exact fp32
 * throughout (no precision switch).  Activations are channels-last, [B, T_l, F_l, C_l], sizes L -> (L - 1) / 2 + 1 per stage
 * on both axes.
 * ------------------------------------------------------------------------------------- */
#define TTSENC_STYLE_MAX_CONVS 8
enum { TTSENC_STYLE_ENCODER = 0, TTSENC_STYLE_VAE = 1, TTSENC_STYLE_GST = 2, TTSENC_STYLE_GST_VAE = 3 };
typedef struct ttsenc_style_dims {
  int32_t n_mels;                            /* audio.num_mels: the input's feature axis                              */
  int32_t n_convs;                           /* len(ref_enc_filters) (6), 1 .. TTSENC_STYLE_MAX_CONVS                  */
  int32_t filters[TTSENC_STYLE_MAX_CONVS];   /* ref_enc_filters (32, 32, 64, 64, 128, 128): multiples of 4             */
  int32_t d_enc;                             /* ReferenceEncoder dim_out (128): LSTM hidden size, a multiple of 4      */
  int32_t kind;                              /* TTSENC_STYLE_*                                                         */
  int32_t d_emb;                             /* dim_emb (256): the style embedding added to `memory` (kinds 1 - 3)     */
  int32_t d_vae;                             /* dim_vae (kinds 1, 3)                                                   */
  int32_t n_tokens;                          /* num_tokens (kinds 2, 3), <= 64                                         */
  int32_t n_heads;                           /* num_heads (kinds 2, 3), <= 16, divides d_emb                           */
  float bn_eps;                              /* 1e-5                                                                   */
} ttsenc_style_dims;
typedef struct ttsenc_style_handle ttsenc_style_handle;

/* Source tensors for ttsenc_style_pack_weights: the head in this order, then six per conv stage i at
 * TTSENC_STYLE_W_STAGES + 6 * i + TTSENC_STYLE_W_CONV_W ... (ttsenc_style_num_weight_tensors = TTSENC_STYLE_W_STAGES +
 * 6 * n_convs).  Tensors that the handle's kind does not have are NULL. */
enum {
  TTSENC_STYLE_W_LSTM_IH = 0, /* encoder.gru.weight_ih_l0 [4 d_enc, C_last * F_last], columns c * F_last + f       */
  TTSENC_STYLE_W_LSTM_HH,     /* encoder.gru.weight_hh_l0 [4 d_enc, d_enc]                                          */
  TTSENC_STYLE_W_LSTM_BIH,    /* encoder.gru.bias_ih_l0 [4 d_enc]                                                   */
  TTSENC_STYLE_W_LSTM_BHH,    /* encoder.gru.bias_hh_l0 [4 d_enc]                                                   */
  TTSENC_STYLE_W_MEAN_W,      /* mean_linear.weight [d_vae, d_enc (VAE) or d_emb (GST_VAE)]                         */
  TTSENC_STYLE_W_MEAN_B,      /* mean_linear.bias [d_vae]                                                           */
  TTSENC_STYLE_W_LOGVAR_W,    /* logvar_linear.weight                                                               */
  TTSENC_STYLE_W_LOGVAR_B,    /* logvar_linear.bias                                                                 */
  TTSENC_STYLE_W_FC_OUT,      /* fc_out.weight [d_emb, d_vae]                                                       */
  TTSENC_STYLE_W_EMBED,       /* stl.embed [n_tokens, d_emb / n_heads]                                              */
  TTSENC_STYLE_W_QUERY,       /* stl.attention.W_query.weight [d_emb, d_enc]                                        */
  TTSENC_STYLE_W_KEY,         /* stl.attention.W_key.weight [d_emb, d_emb / n_heads]                                */
  TTSENC_STYLE_W_VALUE,       /* stl.attention.W_value.weight [d_emb, d_emb / n_heads]                              */
  TTSENC_STYLE_W_STAGES       /* first tensor of conv stage 0                                                       */
};
enum {
  TTSENC_STYLE_W_CONV_W = 0,  /* encoder.convs.i.weight [C_i, C_{i-1}, 3, 3]                                        */
  TTSENC_STYLE_W_CONV_B,      /* encoder.convs.i.bias [C_i]                                                         */
  TTSENC_STYLE_W_BN_W,        /* encoder.bns.i.weight                                                               */
  TTSENC_STYLE_W_BN_B,        /* encoder.bns.i.bias                                                                 */
  TTSENC_STYLE_W_BN_MEAN,     /* encoder.bns.i.running_mean                                                         */
  TTSENC_STYLE_W_BN_VAR,      /* encoder.bns.i.running_var                                                          */
  TTSENC_STYLE_W_PER_STAGE
};

/* TTSDEC_ERR_DIMS: a filter count that is no multiple of 4, d_enc no multiple of 4 (the LSTM kernel's K segments are 16-byte
 * columns), d_emb % n_heads != 0, or a size beyond the limits above. */
int ttsenc_style_create(const ttsenc_style_dims* dims, ttsenc_style_handle** out);
int ttsenc_style_destroy(ttsenc_style_handle* h);
const char* ttsenc_style_last_hip_error(const ttsenc_style_handle* h);
int ttsenc_style_num_weight_tensors(const ttsenc_style_handle* h);
size_t ttsenc_style_packed_bytes(const ttsenc_style_handle* h);
/* Besides the copies: conv weights to [C_out][ky][kx][C_in], BatchNorm folded to (alpha, beta), W_ih's columns permuted to the
 * channels-last order f * C + c, b_ih + b_hh, and the token keys / values tanh(embed) . W_key^T, . W_value^T (input-independent). */
int ttsenc_style_pack_weights(ttsenc_style_handle* h, const float* const* src, int n_src, void* blob, void* stream);
int ttsenc_style_bind_weights(ttsenc_style_handle* h, const void* blob);
/* 0 for a (B, T) beyond the size limit stated at ttsdec_workspace_bytes. */
size_t ttsenc_style_workspace_bytes(const ttsenc_style_handle* h, int B, int T);
/* x: frame (b, t) at x + (b * T + t) * ldx, n_mels floats (ldx >= n_mels, a multiple of 4 is not required).
 * lengths [B] int32 on the device or NULL (every row runs all T' = T after n_convs stages steps); a row's LSTM runs
 * min(max(lengths[b] >> n_convs, 1), T') steps - a length above T is clamped here, the caller checks host-side lengths.
 * The convs are not masked: they see whatever the padded frames hold, as the reference's do.
 * eps [B, d_vae] (kinds 1, 3; NULL otherwise): the caller's standard-normal draw.
 * enc_out [B, d_enc] (always); x_out [B, d_emb] and kl_out [B, d_vae] (kinds 1, 3; x_out alone for kind 2; NULL otherwise).
 * No host synchronisation; every reduction runs in a fixed order. */
int ttsenc_style_forward(ttsenc_style_handle* h, const float* x, int ldx, const int32_t* lengths, const float* eps, int B, int T,
                         float* enc_out, float* x_out, float* kl_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * VITS2 second hot path (BASELINE.json configs[4]):
 *   ttsvits_text_encoder  = TextEncoder.forward, vits2/models.py:369-380
 *       (attentions.Encoder :76-93, MultiHeadAttention.attention :246-295 with the relative-position
 *        window :297-368, FFN :411-419, modules.LayerNorm modules.py:24-27)
 *   ttsvits_flow_reverse  = ResidualCouplingTransformersBlock.forward(reverse=True), models.py:803-810
 *       over ResidualCouplingTransformersLayer.forward, models.py:506-531 (mean-only), with
 *       modules.WN.forward modules.py:185-210, commons.fused_add_tanh_sigmoid_multiply commons.py:102-109
 *       and modules.Flip modules.py:374-381.
 * Eval mode, no speaker conditioning (g = None), split-fp16 GEMMs (fp32-class accuracy: hi+lo fp16 planes, fp32 accumulate), fp32 elsewhere.  Activations at this boundary are
 * CHANNEL-LAST: [B, T, C] (the reference's [B, C, T] transposed).
 * ------------------------------------------------------------------------------------- */
typedef struct ttsvits_dims {
  int32_t n_vocab;          /* len(symbols)                                              */
  int32_t inter_channels;   /* 192: flow channels; TextEncoder emits m, logs of this width */
  int32_t hidden_channels;  /* 192                                                       */
  int32_t filter_channels;  /* 768                                                       */
  int32_t n_heads;          /* 2                                                         */
  int32_t n_layers;         /* 6                                                         */
  int32_t kernel_size;      /* 3 (FFN convs of the text encoder)                         */
  int32_t window_size;      /* 4 (relative-position window; heads share the tables)      */
  int32_t flow_hidden;      /* 192: WN width                                             */
  int32_t flow_kernel;      /* 5:   WN conv taps (dilation_rate 1)                       */
  int32_t flow_wn_layers;   /* 4                                                         */
  int32_t n_flows;          /* 4 coupling layers (each followed by a Flip)               */
  int32_t flow_tf_layers;   /* 2: pre_transformer = Encoder(half, half, 2 heads, 2 layers, k=3, no window) */
  int32_t flow_tf_heads;    /* 2                                                         */
  int32_t flow_tf_kernel;   /* 3                                                         */
  int32_t gin_channels;     /* 0, or the speaker-embedding width (a multiple of 4): each coupling layer's WN gets cond_layer
                             * (modules.py:149-153) and the text encoder spk_emb_linear (attentions.py:42-46)                */
  int32_t cond_layer_idx;   /* text-encoder layer at whose input the projected embedding is added (attentions.py:47-52: 2
                             * unless configured); read only when gin_channels > 0 and n_layers > 0                           */
} ttsvits_dims;
typedef struct ttsvits_handle ttsvits_handle;

/* Source tensors for ttsvits_pack_weights (device fp32, the reference's parameter shapes), in this order:
 *   enc_p.emb.weight;
 *   when gin_channels > 0: enc_p.encoder.spk_emb_linear.{weight,bias};
 *   per text-encoder layer i: attn_layers.i.conv_{q,k,v,o}.{weight,bias} (8), emb_rel_k, emb_rel_v,
 *       norm_layers_1.i.{gamma,beta}, ffn_layers.i.conv_1.{weight,bias}, conv_2.{weight,bias},
 *       norm_layers_2.i.{gamma,beta}                                            (18 per layer);
 *   enc_p.proj.{weight,bias};
 *   per coupling layer f (flow.flows.{2f}): per pre_transformer layer the same 16 tensors without the
 *       emb_rel pair; pre.{weight,bias}; when gin_channels > 0: enc.cond_layer EFFECTIVE weight [2*flow_hidden*
 *       flow_wn_layers, gin(, 1)], bias; per WN layer j: in_layers.j EFFECTIVE weight (g*v/||v||), bias,
 *       res_skip_layers.j effective weight, bias; post.{weight,bias}.
 * A NULL entry leaves that tensor zero (a module that owns only the text encoder or only the flow). */
int ttsvits_create(const ttsvits_dims* dims, ttsvits_handle** out);
int ttsvits_destroy(ttsvits_handle* h);
/* Arithmetic of every GEMM of the two entry points below: TTSDEC_PREC_F32 (default: exact fp32 matrix instruction, the
 * reference's own arithmetic) or TTSDEC_PREC_SPLIT_F16 (hi + lo fp16 planes, fp32 accumulate: opt-in, ~1.8x faster); both forms
 * of the weights live in the packed blob, so this can be switched at any time.  The elementwise math is fp32 in both modes;
 * the flow's attention runs on the f16 flash kernel in split mode and on exact-fp32 MFMAs otherwise. */
int ttsvits_set_precision(ttsvits_handle* h, int precision);
int ttsvits_get_precision(const ttsvits_handle* h);
const char* ttsvits_last_hip_error(const ttsvits_handle* h);
int ttsvits_num_weight_tensors(const ttsvits_handle* h);
size_t ttsvits_packed_bytes(const ttsvits_handle* h);
int ttsvits_pack_weights(ttsvits_handle* h, const float* const* src, int n_src, void* blob, void* stream);
int ttsvits_bind_weights(ttsvits_handle* h, const void* blob);
size_t ttsvits_text_encoder_workspace_bytes(const ttsvits_handle* h, int B, int T);
/* ids [B, T] int64, lengths [B] int32 (device).  x [B, T, hidden], m and logs [B, T, inter]; padded frames are zero.
 * g: NULL, or the speaker embedding [B, gin_channels] fp32 (device) - the reference's g [B, gin, 1] (models.py:369, 376;
 * attentions.py:80-84); TTSDEC_ERR_INVALID_ARG when g is given and the handle has gin_channels == 0.
 * status: as for ttsenc_forward (bit 0: an id outside [0, n_vocab), models.py:370).
 * TTSDEC_ERR_DIMS for B * T > INT32_MAX / 4096 frames: the GEMM core counts rows and offsets in 32 bits. */
int ttsvits_text_encoder(ttsvits_handle* h, const int64_t* ids, const int32_t* lengths, const float* g, int B, int T, float* x,
                         float* m, float* logs, void* workspace, size_t workspace_bytes, void* stream, int32_t* status);
size_t ttsvits_flow_workspace_bytes(const ttsvits_handle* h, int B, int T);
/* z [B, T, inter] -> out [B, T, inter]; lengths [B] int32 (device) give y_mask.  g: NULL or the speaker embedding
 * [B, gin_channels] (the reference's g [B, gin, 1], models.py:506, 511; modules.py:185-199), as above.
 * TTSDEC_ERR_DIMS for B * T > INT32_MAX / 4096 frames, as ttsvits_text_encoder. */
int ttsvits_flow_reverse(ttsvits_handle* h, const float* z, const int32_t* lengths, const float* g, int B, int T, float* out,
                         void* workspace, size_t workspace_bytes, void* stream);
/* The forward direction, ResidualCouplingTransformersBlock.forward(reverse=False) (models.py:803-806) over
 * ResidualCouplingTransformersLayer.forward (models.py:506-526, mean-only: x1 = m + x1 * exp(0) * x_mask) - the `self.flow(z, y_mask,
 * g=g_src)` of SynthesizerTrn.voice_conversion, models.py:1334.  Flows run layer_0, Flip, layer_1, Flip, ..., layer_{n-1}, Flip.
 * Same tensors, workspace (ttsvits_flow_workspace_bytes), precisions and errors (TTSDEC_ERR_DIMS for B * T > INT32_MAX / 4096 frames
 * among them) as ttsvits_flow_reverse; the logdet of the training forward is not computed (mean-only: it is 0). */
int ttsvits_flow_forward(ttsvits_handle* h, const float* z, const int32_t* lengths, const float* g, int B, int T, float* out,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Monotonic alignment search between the text encoder's prior and the flow's z_p (the inverse of the length regulation,
 * ttsdur_lengths / ttsdur_expand): the `with torch.no_grad():` block of SynthesizerTrn.forward (models.py:1224-1254) and
 * monotonic_align/core.pyx:7-33.  Weightless: like ttsdur_lengths / ttsdur_expand these calls use the handle (of any dims, bound
 * or not) for its device and its error text only.  They enqueue only.
 *   t_y, t_x [B] int32 (device): frames and tokens of each utterance (the reference's mask.sum(1)[:, 0] / mask.sum(2)[:, 0]).
 *   T_x <= 1024 (any T_y); more is refused with TTSDEC_ERR_DIMS. */
enum { TTSVITS_PATH_F32 = 0, TTSVITS_PATH_F16 = 1, TTSVITS_PATH_BF16 = 2 }; /* element type of the dense path */
/* Scratch of one ttsvits_maximum_path / ttsvits_align call: one decision bit per cell of the search (256-byte aligned). */
size_t ttsvits_align_workspace_bytes(const ttsvits_handle* h, int B, int T_y, int T_x);
/* neg_cent [B, T_y, T_x] (models.py:1226-1239) from z_p [B, T_y, C], m_p / logs_p [B, T_x, C], channel-last fp32, 16-byte aligned,
 * C a multiple of 4 up to 4096:  sum_d(-0.5 log 2pi - logs_p) + sum_d(-0.5 z_p^2 s) + sum_d(z_p m_p s) + sum_d(-0.5 m_p^2 s) with
 * s = exp(-2 logs_p); the two middle terms are one 2C-deep contraction in exact fp32 on the matrix pipe.  Cells at or beyond
 * t_y[b] x t_x[b] are written as zeros; t_y / t_x NULL: every utterance is T_y x T_x. */
int ttsvits_neg_cent(ttsvits_handle* h, const float* z_p, const float* m_p, const float* logs_p, const int32_t* t_y, const int32_t* t_x, int B,
                    int T_y, int T_x, int C, float* neg_cent, void* stream);
/* monotonic_align.maximum_path on any neg_cent [B, T_y, T_x] fp32 (not modified): the reference's path, bit for bit (fp32 `+` and
 * max in its order, its edge rules, a tie stays on the token).
 *   path        NULL, or [B, T_y, T_x] of path_dtype: 1 on the path, 0 elsewhere (zeros outside t_y x t_x)
 *   frame_token [B, T_y] int32: the token of every frame, -1 at frames >= t_y[b]
 *   dur         [B, T_x] int32: frames per token (path.sum over frames), 0 at tokens >= t_x[b]
 *   status      [1] int32: 0, or flags of the utterances that were refused because the reference reads out of bounds there:
 *               1 = t_y < 1 or t_x < 1, 2 = t_y < t_x, 4 = t_y > T_y or t_x > T_x.  Such an utterance gets frame_token -1, dur 0 and a
 *               zero path; the caller reads status once and discards the call's outputs when it is not 0. */
int ttsvits_maximum_path(ttsvits_handle* h, const float* neg_cent, const int32_t* t_y, const int32_t* t_x, int B, int T_y, int T_x, void* path,
                        int path_dtype, int32_t* frame_token, int32_t* dur, int32_t* status, void* workspace, size_t workspace_bytes,
                        void* stream);
/* ttsvits_neg_cent into neg_cent [B, T_y, T_x] (kept: the caller's buffer), then ttsvits_maximum_path on it. */
int ttsvits_align(ttsvits_handle* h, const float* z_p, const float* m_p, const float* logs_p, const int32_t* t_y, const int32_t* t_x, int B, int T_y,
                 int T_x, int C, float* neg_cent, void* path, int path_dtype, int32_t* frame_token, int32_t* dur, int32_t* status,
                 void* workspace, size_t workspace_bytes, void* stream);

/* Spectrogram front-end: the reference's vits2/mel_processing.py:58-187 (spectrogram_torch, spec_to_mel_torch, mel_spectrogram_torch,
 * center=False), from waveforms to what ttspost_forward reads.  Weightless like the alignment calls above: the handle (of any dims,
 * bound or not) gives its device and its error text.  The calls enqueue only.
 *   wav      [B, N] fp32, one utterance per row; lengths [B] int32 samples of each (device), or NULL: every row is N samples
 *   window   [win_size] fp32 (the reference's torch.hann_window(win_size)), centred in the n_fft-point frame with zeros around it
 *   n_fft    256, 512, 1024 or 2048 (else TTSDEC_ERR_DIMS); win_size <= n_fft; any hop_size >= 1; bins = n_fft / 2 + 1
 *   An utterance of len samples is reflect-padded by pad = (n_fft - hop_size) / 2 (C division) at its own two ends and has
 *   1 + (len + 2 pad - n_fft) / hop_size frames; frame t, bin k is sqrt(re^2 + im^2 + 1e-6) of the windowed n_fft-point DFT of the
 *   padded samples from t * hop_size (an FFT in fp32, twiddles evaluated in fp64 and rounded once).
 *   T        frames of the output tensors; frames at or past an utterance's count are written as exact zeros
 *   status   NULL, or [1] int32 (device): 0, or flags of refused utterances, whose frames are all zeros: 1 = len <= pad (the
 *            reflection is undefined), 2 = no frame (len + 2 pad < n_fft), 4 = len > N or more frames than T (clamped)
 *   mel_basis [n_mels, bins] fp32 row-major, n_mels <= 256: mel = log(max(mel_basis @ spec, 1e-5)) with fp32 sums over each row's
 *            run of non-zero entries, in bin order
 *   workspace ttsvits_spec_workspace_bytes(h, n_fft, n_mels) bytes (n_mels = 0 for ttsvits_spectrogram), 256-byte aligned; every call
 *            rebuilds its tables there (twiddles; the non-zero run of each basis row) with one small launch of its own.
 * Sizes are checked before any pointer: TTSDEC_ERR_INVALID_ARG for a size <= 0, TTSDEC_ERR_DIMS as above, then NULL pointers,
 * then TTSDEC_ERR_WORKSPACE. */
size_t ttsvits_spec_workspace_bytes(const ttsvits_handle* h, int n_fft, int n_mels); /* 0: n_fft or n_mels outside the ranges above */
/* spec [B, bins, T] */
int ttsvits_spectrogram(ttsvits_handle* h, const float* wav, const int32_t* lengths, int B, int N, const float* window, int n_fft, int hop_size,
                        int win_size, float* spec, int T, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
/* mel [B, n_mels, T] from spec [B, bins, T] (bins = n_fft / 2 + 1); frames [B] int32 (device) or NULL: zeros at frames >= frames[b] */
int ttsvits_spec_to_mel(ttsvits_handle* h, const float* spec, const int32_t* frames, int B, int n_fft, int T, const float* mel_basis, int n_mels,
                        float* mel, void* workspace, size_t workspace_bytes, void* stream);
/* mel [B, n_mels, T] from the waveforms: ttsvits_spectrogram and ttsvits_spec_to_mel in one kernel, the magnitudes staying in LDS */
int ttsvits_mel_spectrogram(ttsvits_handle* h, const float* wav, const int32_t* lengths, int B, int N, const float* window, int n_fft, int hop_size,
                            int win_size, const float* mel_basis, int n_mels, float* mel, int T, int32_t* status, void* workspace,
                            size_t workspace_bytes, void* stream);

/* The glue of the validation step: what SynthesizerTrn.forward (models.py:1269-1276) and the trainer (train.py:357-373, 416-418) do
 * between the encoders, the alignment, the generator and the loss terms - the prior expanded along the alignment, losses.kl_loss
 * (losses.py:37-46), commons.slice_segments (commons.py:50-56) and F.l1_loss on a slice.  Weightless like the alignment calls: the
 * handle (of any dims, bound or not) gives its device and its error text.  The calls enqueue only.  Exact fp32; every sum has a
 * fixed order (no atomics), so a call repeats bit for bit and an utterance's own sum does not depend on the batch around it.
 * Sizes are checked before any pointer: TTSDEC_ERR_INVALID_ARG for a size <= 0, TTSDEC_ERR_DIMS beyond the limits below, then NULL
 * (or misaligned) pointers, then TTSDEC_ERR_WORKSPACE.  B <= 65535; tensors of up to 2^31 elements. */
/* Scratch of one ttsvits_kl_loss call: one partial sum per frame (256-byte aligned); 0 for a NULL handle or a size <= 0. */
size_t ttsvits_kl_loss_workspace_bytes(const ttsvits_handle* h, int B, int T_y);
/* kl_loss(z_p, logs_q, m_p, logs_p, y_mask) with the prior still per token, in one pass over the four operands:
 *   z_p, logs_q  [B, T_y, C] channel-last fp32, 16-byte aligned; C a multiple of 4 up to 4096 (as ttsvits_neg_cent)
 *   m_p, logs_p  [B, T_x, C] channel-last, unexpanded
 *   frame_token  [B, T_y] int32 as ttsvits_maximum_path writes it (-1: no token), or NULL: the prior is per frame already
 *                (T_x == T_y, else TTSDEC_ERR_INVALID_ARG)
 *   t_y          [B] int32 (device): frames of each utterance; frames at or past it do not count
 *   m_p_exp, logs_p_exp   each NULL, or [B, T_y, C]: the token's row at every frame, exact zeros where a frame has no token -
 *                what the reference's two matmuls by the one-hot path give (models.py:1270-1271); the losses never read them
 *   kl_rows      [B]: each utterance's sum of logs_p - logs_q - 0.5 + 0.5 (z_p - m_p)^2 exp(-2 logs_p) over its t_y[b] x C elements
 *   kl           [2]: the sum of kl_rows, and that sum / sum(t_y) - the reference's kl_loss (its divisor counts frames, not
 *                frames x channels)
 * Sums go per frame (one wave, lane order), then per utterance over its own t_y[b] frame sums, then over the batch. */
int ttsvits_kl_loss(ttsvits_handle* h, const float* z_p, const float* logs_q, const float* m_p, const float* logs_p, const int32_t* frame_token,
                    const int32_t* t_y, int B, int T_y, int T_x, int C, float* m_p_exp, float* logs_p_exp, float* kl_rows, float* kl,
                    void* workspace, size_t workspace_bytes, void* stream);
/* commons.slice_segments as one launch with no host read: x is viewed as [B, outer, T, inner] fp32, ids is [B] int64 (ids_int64 != 0)
 * or int32 (device), and out[b, o, t, i] = x[b, o, ids[b] * scale + t, i] for t < seg, out [B, outer, seg, inner].  The view serves a
 * channel-last z (outer 1, inner C), a channel-first mel (outer n_mels, inner 1) and a waveform (outer = inner = 1, scale = hop).
 * seg <= T (else TTSDEC_ERR_DIMS), scale >= 1.  16-byte loads are used only where inner is a multiple of 4 and x and out are 16-byte
 * aligned; any alignment is accepted.
 *   status  [1] int32 (device): 0, or 1 when some ids[b] * scale is below 0 or beyond T - seg (the reference raises a shape error
 *           there); that utterance's slice is exact zeros. */
int ttsvits_slice_segments(ttsvits_handle* h, const float* x, const void* ids, int ids_int64, int B, int outer, int T, int inner, int seg, int scale,
                           float* out, int32_t* status, void* stream);
/* F.l1_loss(slice_segments(a, ids, seg), y) without the slice in memory: a [B, C, T_a], y [B, C, seg] fp32, ids as above, or NULL:
 * plain L1 of two tensors of one shape (seg == T_a, else TTSDEC_ERR_INVALID_ARG).
 *   l1_rows [B]: each utterance's sum of |a[b, c, ids[b] + t] - y[b, c, t]| over its C x seg elements
 *   l1      [2]: the sum of l1_rows, and that sum / (B C seg) - the reference's mean
 *   status  as for ttsvits_slice_segments (an utterance out of range counts as a slice of zeros) */
int ttsvits_sliced_l1(ttsvits_handle* h, const float* a, const float* y, const void* ids, int ids_int64, int B, int C, int T_a, int seg,
                      float* l1_rows, float* l1, int32_t* status, void* stream);

/* Mel -> waveform for the Tacotron path: the reference's tacotron/inference.py:13-22 (synth_audio) with AudioFrontend.mel_inv /
 * .decode (tacotron/data/audio.py:69-76) and m_rev (tacotron/data/dataset.py:183-184) - torchaudio's InverseMelScale,
 * amplitude_to_DB, DB_to_amplitude and GriffinLim - on a padded batch.  Weightless: the ttsdec handle (of any dims, bound or not)
 * gives its device and its error text.  The calls enqueue only.  Exact fp32.
 *   frames   [B] int32 mel frames of each utterance (device), or NULL: every row has T.  An utterance of T_b frames gives
 *            hop_length * (T_b - 1) samples (torch.istft(center=True)); frames at or past T_b and samples at or past that count are
 *            written as exact zeros.  T >= 2.
 *   n_fft    256, 512, 1024 or 2048 (else TTSDEC_ERR_DIMS), win_length == n_fft; hop_length <= n_fft / 2 (else TTSDEC_ERR_DIMS: the
 *            overlap-added squared window must have no zero); bins = n_fft / 2 + 1
 *   status   NULL, or [1] int32 (device): 0, or flags: 1 = an utterance of fewer than 2 frames (its row is zeros), 4 = frames[b] > T
 *            (clamped)
 * Sizes are checked before any pointer: TTSDEC_ERR_INVALID_ARG for a size <= 0, TTSDEC_ERR_DIMS as above, then NULL pointers,
 * then TTSDEC_ERR_WORKSPACE. */
size_t ttsdec_griffinlim_workspace_bytes(const ttsdec_handle* h, int B, int T, int n_fft); /* 0: a size outside the ranges above */
/* y [B, T, n_mels] (the model's normalised mel, n_mels <= 256) -> mag [B, bins, T], the magnitude Griffin-Lim starts from:
 *   M = 10^(0.1 (100 y - 100))                      m_rev, then db_to_amplitude (audio.py:74, dataset.py:183-184)
 *   D = relu(P M)                                   InverseMelScale (audio.py:75): P [bins, n_mels] fp32 row-major is the minimum-norm
 *                                                   solution operator fb (fb^T fb)^-1 of fb^T D = M - what lstsq(driver="gels")
 *                                                   solves per utterance in the reference - for the filterbank fb [bins, n_mels]
 *   mag = sqrt(10^(0.1 * 10 log10(max(D, 1e-12))))  amplitude_to_db (audio.py:76), db_to_amplitude (audio.py:70), and the
 *                                                   root GriffinLim(power=2) takes first; a zero of D gives 1e-6
 * with fp32 sums over the n_mels terms in order. */
int ttsdec_mel_to_magnitude(ttsdec_handle* h, const float* y, const float* P, const int32_t* frames, int B, int T, int n_mels, int n_fft, float* mag,
                            int32_t* status, void* stream);
/* mag [B, bins, T] -> wave [B, hop_length * (T - 1)] by n_iter iterations of fast Griffin-Lim (audio.py:59-65, :71; torchaudio
 * functional.griffinlim on the magnitude, i.e. after its pow(1 / power)):
 *   repeat n_iter times:  inverse = istft(mag * angles);  rebuilt = stft(inverse, center=True, pad_mode="reflect");
 *                         angles = rebuilt - tprev * momentum / (1 + momentum);  angles /= |angles| + 1e-16;  tprev = rebuilt
 *   wave = istft(mag * angles), and with normalize != 0 wave / max |wave| per utterance (inference.py:21)
 *   window   [n_fft] fp32 (the reference's torch.hann_window(n_fft))
 *   angles   NULL (all ones: rand_init=False), or the initial phase factors [B, bins, T] complex64 (interleaved re, im) - torchaudio
 *            starts from complex(rand, rand), which is not of unit modulus; the caller draws it
 *   tprev    NULL (zeros), or [B, bins, T] complex64: with angles, the state of an iteration to go on from
 *   0 <= momentum < 1;  n_iter >= 0 (0: the inverse STFT alone)
 *   rebuilt_out, angles_out  NULL, or [B, bins, T] complex64 (n_iter >= 1 only): the last rebuilt spectrum (the next tprev) and the
 *            phase factors the waveform was made from
 *   An utterance of no more than n_fft / 2 samples is reflected as often as the padding needs (torch.stft refuses it).
 *   workspace ttsdec_griffinlim_workspace_bytes(h, B, T, n_fft) bytes, 256-byte aligned; holds the twiddles (rebuilt by every call),
 *            the frame-major magnitude, two spectra and the windowed inverse frames [B, T, n_fft].
 * Deterministic: no atomics in the overlap-add; every utterance gets bit for bit what it gets alone. */
int ttsdec_griffinlim(ttsdec_handle* h, const float* mag, const int32_t* frames, int B, int T, const float* window, int n_fft, int hop_length,
                      const float* angles, const float* tprev, int n_iter, float momentum, int normalize, float* wave, float* rebuilt_out,
                      float* angles_out, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* Waveform -> dB spectrogram and dB mel for the Tacotron path: the reference's AudioFrontend.encode (tacotron/data/audio.py:55-67)
 * after its resampling - wave / max |wave|, torchaudio's Spectrogram(power=2, normalized=True, center=True), MelScale and
 * amplitude_to_DB(10, 1e-12, 0) - on a padded batch.  Weightless like the calls above; enqueues only.  Exact fp32.
 *   wave     [B, n_samples] fp32, one utterance per row; lengths [B] int32 samples of each (device), or NULL: every row is n_samples
 *   window   [n_fft] fp32 (the reference's torch.hann_window(n_fft)); fb [bins, n_mels] fp32 row-major, the mel filterbank
 *   n_fft    256, 512, 1024 or 2048, win_length == n_fft; 1 <= hop_length <= n_fft / 2 (the range of ttsdec_griffinlim, its
 *            inverse); n_mels <= 256; B <= 65535; 1 <= T <= 2^22; n_samples <= 2^30 (else TTSDEC_ERR_DIMS); bins = n_fft / 2 + 1
 *   An utterance of len samples is divided by its own max |x|, reflect-padded by n_fft / 2 at its own two ends and has
 *   1 + len / hop_length frames (C division).  Frame t:
 *     D[k] = |X[k]|^2 / sum w^2                 X the windowed n_fft-point DFT of the padded samples from t * hop_length (an FFT in
 *                                               fp32, twiddles and 1 / sum w^2 evaluated in fp64 and rounded once)
 *     M[m] = sum_k fb[k, m] D[k]                fp32 sums over each filter's run of non-zero entries, in bin order
 *     spec_db = 10 log10(max(D, 1e-12)),  mel_db = 10 log10(max(M, 1e-12))
 *   D itself never reaches memory.
 *   T        frames of the output tensors; frames at or past an utterance's count are written as exact zeros
 *   spec_db  NULL (not computed), or [B, T, bins];  mel_db [B, T, n_mels];  frames_out NULL, or [B] int32: every utterance's frames
 *   status   NULL, or [1] int32 (device): 0, or flags of refused utterances, whose frames are all zeros and whose count is 0:
 *            1 = len <= n_fft / 2 (the reflection is undefined), 2 = max |x| is 0 (the reference divides by it); and
 *            4 = len > n_samples or more frames than T (clamped)
 *   workspace ttsdec_mel_analysis_workspace_bytes(h, B, n_fft, n_mels) bytes, 256-byte aligned; every call rebuilds its tables there
 *            (twiddles, the bands of the filterbank, 1 / sum w^2) and keeps the peaks there.
 * Sizes are checked before any pointer: TTSDEC_ERR_INVALID_ARG for B, n_samples or n_mels <= 0, TTSDEC_ERR_DIMS as above, then NULL
 * pointers, then TTSDEC_ERR_WORKSPACE.  Deterministic (the peak is an integer maximum); every utterance gets bit for bit what it
 * gets alone. */
size_t ttsdec_mel_analysis_workspace_bytes(const ttsdec_handle* h, int B, int n_fft, int n_mels); /* 0: a size outside the ranges above */
int ttsdec_mel_analysis(ttsdec_handle* h, const float* wave, const int32_t* lengths, int B, int n_samples, const float* window, const float* fb,
                        int n_mels, int n_fft, int hop_length, int T, float* spec_db, float* mel_db, int32_t* frames_out, int32_t* status,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Sample-rate conversion of a padded batch: torchaudio's functional.resample with its defaults (sinc_interp_hann), the first line of
 * the reference's AudioFrontend.encode (tacotron/data/audio.py:55-58).  Weightless like the calls above; enqueues only.  Exact fp32.
 * With g = gcd(orig_freq, new_freq), o = orig_freq / g, n = new_freq / g and lpw = lowpass_filter_width:
 *     base  = min(o, n) * rolloff,   width = ceil(lpw * o / base),   taps = 2 * width + o
 *     t     = clamp(base * ((k - width) / o - p / n), -lpw, +lpw)                          phase p < n, tap k < taps
 *     K[p, k] = (base / o) * cos(t * pi / lpw / 2)^2 * (t == 0 ? 1 : sin(pi t) / (pi t))   in fp64, rounded once
 *     y[blk * n + p] = sum_k K[p, k] * xp[blk * o + k]         xp: the utterance with width zeros in front of it and zeros after it
 *   wave     [B, n_samples] fp32, one utterance per row; lengths [B] int32 samples of each (device), or NULL: every row is n_samples.
 *            Samples at or past lengths[b] count as zero whatever the row holds there (they are never read).
 *   out      [B, n_out] fp32: utterance b has ceil(n * len_b / o) samples (64-bit integers), exact zeros after them up to n_out;
 *            lengths_out NULL, or [B] int32: those counts
 *   status   NULL, or [1] int32 (device): 0, or 4 = lengths[b] > n_samples or more output than n_out (clamped)
 *   workspace ttsdec_resample_workspace_bytes(...) = align256(4 * n * taps) bytes, 256-byte aligned: the table alone, which every call
 *            rebuilds there in fp64 with one launch.  Where t is clamped the rounded K is an exact zero (cos(pi / 2)^2 ~ 4e-33), so the
 *            table keeps, per phase, only the run of taps around width + o p / n that can be non-zero, and a sum runs over that run.
 *   rolloff  is read as the 7-digit decimal that gives this float (0.99f as 0.99), in fp64 like everything else of the table
 *   orig_freq != new_freq, both > 0; lowpass_filter_width >= 1; 0 < rolloff <= 1 (else TTSDEC_ERR_INVALID_ARG, as for B, n_samples or
 *   n_out <= 0); o <= 1024, n <= 1024, taps <= 16384, B <= 65535, n_samples <= 2^30, n_out <= 2^30 (else TTSDEC_ERR_DIMS: 16001 ->
 *   16000 would need a 1 GB table).  Sizes are checked before any pointer, then NULL pointers, then TTSDEC_ERR_WORKSPACE.
 * Every output is one fp32 fma chain over its taps in tap order: deterministic, and every utterance gets bit for bit what it gets
 * alone.  No atomics but the status word; no host synchronisation. */
size_t ttsdec_resample_workspace_bytes(const ttsdec_handle* h, int orig_freq, int new_freq, int lowpass_filter_width, float rolloff);
        /* 0: refused */
int ttsdec_resample(ttsdec_handle* h, const float* wave, const int32_t* lengths, int B, int n_samples, int orig_freq, int new_freq,
                    int lowpass_filter_width, float rolloff, float* out, int n_out, int32_t* lengths_out, int32_t* status,
                    void* workspace, size_t workspace_bytes, void* stream);

/* The loss terms of the Tacotron validation step: what the reference's run_training_step (tacotron/tacotron.py:100-138) and
 * TacotronTask.train_forward (tacotron/tacotron_lightning.py:50-99) compute from the forward's outputs - mel_loss_fn on the frames
 * and on their differences, with and without a mask, the pos_weight BCE on the stop logits, alignment_std_loss and
 * alignment_max_loss.  Weightless like the calls above (the handle gives the device and the error text); enqueues only; exact fp32.
 *   y, y_post [B, T, D] fp32; y_post may be NULL.  y and x may both be NULL: the frame terms are then left out (zero).
 *   x         [B, T_x, D], T_x >= T: only its first T frames count; indexed by its own batch stride (no x[:, :T] copy).
 *   s         [B, T] stop logits, or NULL.
 *   w         [B, S, L] attention weights of the S decoder steps, or NULL (S and L are then ignored).
 *   lengths   [B] int32 frames of each utterance (device), len_b = clamp(lengths[b], 0, T); NULL: every utterance has T frames.
 *   rows      [B, 9] out, the per-utterance sums:
 *               0 / 1  A_y, A_p        sum over t < len_b and d of |y - x| (|y_post - x|)
 *               2 / 3  Dall_y, Dall_p  sum over t < T - 1 and d of |(y[t+1] - y[t]) - (x[t+1] - x[t])|
 *               4 / 5  Dmsk_y, Dmsk_p  the same over t + 1 < len_b
 *               6      BCE             sum over t < T of (1 - z) s + (1 + (pos_weight - 1) z) (log1p(exp(-|s|)) + max(-s, 0)), z = (t < len_b)
 *               7 / 8  V, M            sum over the steps of max(var, 0) and of 1 - max_l w, with S0 = sum_l w, m1 = sum_l w l and
 *                                      var = sum_l w (l - m1)^2 + m1^2 (1 - S0): the reference's sum w l^2 - (sum w l)^2, without the
 *                                      cancellation of that form in fp32
 *   terms     [16] out; with N = sum_b len_b and N1 = sum_b max(len_b - 1, 0):
 *               0 / 1  mel, mel_post            sum A / (D N)                 mel_loss_fn(., x, xmask, 1)
 *               2 / 3  dmel_all, dmel_post_all  sum Dall / (B (T - 1) D)      run_training_step's unmasked difference term
 *               4 / 5  dmel, dmel_post          sum Dmsk / (D N1)             TacotronTask's xmask[:, 1:] form
 *               6      stop                     sum BCE / (B T)
 *               7      w_std                    sqrt(sum V / (B S))
 *               8      w_max                    sum M / (B S)
 *               9 / 10 N, N1 as floats;  11 .. 15 zero, as are the terms of an operand that is NULL
 *             A divisor of zero gives NaN, as the reference's 0 / 0 does: terms 0 and 1 when every length is 0, terms 4 and 5
 *             when no length exceeds 1, terms 2 and 3 when T = 1.  The other terms are unaffected.
 *   workspace ttsdec_val_losses_workspace_bytes(h, B, T, S) bytes (S = 0 without w), 256-byte aligned: the per-frame and per-step
 *             sums.  Nothing beyond the reported size is touched.
 * A workgroup of the frame pass owns TTSDEC_VAL_FRAME_RUN consecutive frames of one utterance and reads the one frame behind its
 * run besides: y, y_post and x are read once (the halo frames twice), s and w once.  16-byte loads where D is a multiple of 4 and
 * y, y_post and x are 16-byte aligned, 4-byte loads otherwise, with the same lane-to-channel map: the results do not depend on it.
 * Every sum runs in a fixed order that depends on D, T, S, L and the utterance's own length only: no atomics, a row of `rows` is
 * bit for bit what the utterance gets alone, and a call repeats bit for bit.
 * TTSDEC_ERR_INVALID_ARG for h NULL or a size <= 0 (S, L: with w) or T_x < T; TTSDEC_ERR_DIMS for B > 65535, D > 1024 or a tensor
 * of more than 2^31 elements; then NULL pointers (rows, terms; y without x or x without y; y_post without y; no operand at all);
 * then TTSDEC_ERR_WORKSPACE; then TTSDEC_ERR_DEVICE.
 *
 * ttsdec_mel_loss is the plain form behind mel_loss_fn(y, x, mask, order) (tacotron.py:59-84): order 0 (|y - x| weighted by
 * clip(mean_d x, 0.1) of the frame where y > x), 1 (L1) or 2 (squared error, the root of the mean), over t < len_b with lengths
 * (sum / (D N)) and over every frame without (sum / (B T D)).  rows [B]: the per-utterance sums; out [1].  The same frame pass
 * and the same refusals (order outside 0 .. 2: TTSDEC_ERR_INVALID_ARG); workspace: ttsdec_val_losses_workspace_bytes(h, B, T, 0). */
#define TTSDEC_VAL_FRAME_RUN 32
size_t ttsdec_val_losses_workspace_bytes(const ttsdec_handle* h, int B, int T, int S); /* 0: refused */
int ttsdec_val_losses(ttsdec_handle* h, const float* y, const float* y_post, const float* x, int T_x, const float* s, const float* w,
                      const int32_t* lengths, int B, int T, int D, int S, int L, float pos_weight, float* rows, float* terms,
                      void* workspace, size_t workspace_bytes, void* stream);
int ttsdec_mel_loss(ttsdec_handle* h, const float* y, const float* x, int T_x, const int32_t* lengths, int B, int T, int D, int order,
                    float* rows, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * VITS2 HiFi-GAN generator (latent z -> waveform): Generator.forward, vits2/models.py:900-974, with ResBlock1.forward
 * modules.py:221-315 called without x_mask - the `self.dec(...)` of SynthesizerTrn.infer, models.py:1322.  Eval mode, exact fp32
 * (the fp32-input matrix instruction for every conv, fp32 vector ALU elsewhere; split-fp16 is opt-in per call through
 * ttsvits_generator_forward, at the end of this block).  Activations are CHANNEL-LAST: z [B, T, C].
 *   conv_pre (7 taps) [+ cond(g)]; per upsampling stage i: leaky_relu(0.1), ConvTranspose1d(k = 2u, stride u) as a 3-tap conv
 *   producing u output phases per input frame, then the mean of n_res ResBlock1 (three (dilated conv, conv) pairs each);
 *   leaky_relu(0.01) (models.py:963: the default slope), conv_post (7 taps, no bias), tanh.
 * Every conv is an implicit-im2col GEMM of the library's GEMM core; the leaky ReLUs, residual adds, branch sum and the
 * division by n_res ride in the GEMM epilogues, conv_post + tanh is a streaming kernel (one output sample per lane).
 * Utterances are processed in groups of G = min(B, floor((2^31 - 4096) / (4 F)), floor(65535 * 64 / T')) utterances, F = the
 * largest activation of one utterance in floats (max(T * upsample_initial_channel, max_i T_i * C_i), T_i = T * u_0 * ... * u_i,
 * C_i = upsample_initial_channel >> (i + 1)), T' = T * prod(up_rates): no activation buffer of a launch reaches 2 GiB, no launch
 * has more than 65535 row tiles, and the workspace is sized for one group, not for B (ModelConfig dims at T = 600: F = 4.9 M
 * floats, G = 27).
 * ------------------------------------------------------------------------------------- */
#define TTSGEN_MAX_UP 8
#define TTSGEN_MAX_RES 4
typedef struct ttsgen_dims {
  int32_t initial_channel;          /* inter_channels (192): channels of z                                        */
  int32_t upsample_initial_channel; /* 512; stage i has upsample_initial_channel >> (i + 1) channels (multiples of 4) */
  int32_t n_up;                     /* len(upsample_rates) (4), 1..TTSGEN_MAX_UP                                   */
  int32_t up_rates[TTSGEN_MAX_UP];  /* [8, 8, 2, 2]: even u                                                        */
  int32_t up_kernels[TTSGEN_MAX_UP];/* [16, 16, 4, 4]: k = 2u is the only form built                               */
  int32_t n_res;                    /* len(resblock_kernel_sizes) (3), 1..TTSGEN_MAX_RES                           */
  int32_t res_kernels[TTSGEN_MAX_RES];       /* [3, 7, 11]: odd, <= 31                                             */
  int32_t res_dilations[TTSGEN_MAX_RES][3];  /* [[1, 3, 5]] x 3: 1..16; a dilation > 1 needs stage channels that divide
                                              * 32 or are multiples of 32                                         */
  int32_t n_dil;                    /* dilations per ResBlock1: 3 (the only count built)                           */
  int32_t resblock;                 /* 1 = ResBlock1; 2 (ResBlock2) is not built                                   */
  int32_t gin_channels;             /* 0, or the speaker-embedding width of cond (models.py:944-945)               */
} ttsgen_dims;
typedef struct ttsgen_handle ttsgen_handle;

/* Dimensions not built (ResBlock2, k != 2u or odd u, n_dil != 3, even resblock kernels, channels that are not multiples of 4,
 * ...) are refused with TTSDEC_ERR_DIMS. */
int ttsgen_create(const ttsgen_dims* dims, ttsgen_handle** out);
int ttsgen_destroy(ttsgen_handle* h);
const char* ttsgen_last_hip_error(const ttsgen_handle* h);
/* Source tensors for ttsgen_pack_weights (device fp32, the reference's parameter shapes, EFFECTIVE weights - g * v / ||v|| of
 * weight_norm folded, as after Generator.remove_weight_norm(), models.py:970-974), in this order:
 *   conv_pre.weight [C0, initial_channel, 7], conv_pre.bias [C0];
 *   per stage i: ups.i.weight [C_{i-1}, C_i, k_i] (ConvTranspose1d layout [in, out, k]), ups.i.bias [C_i];
 *   per stage i, per ResBlock1 j (resblocks.{i * n_res + j}): convs1.{0,1,2}.{weight [C_i, C_i, k_j], bias},
 *       then convs2.{0,1,2}.{weight, bias}                                                              (12 per block);
 *   conv_post.weight [1, C_last, 7];
 *   when gin_channels > 0: cond.weight [C0, gin, 1], cond.bias [C0].
 * (C0 = upsample_initial_channel, C_i = C0 >> (i + 1).)  155 tensors at the ModelConfig dims. */
int ttsgen_num_weight_tensors(const ttsgen_handle* h);
size_t ttsgen_packed_bytes(const ttsgen_handle* h);
int ttsgen_pack_weights(ttsgen_handle* h, const float* const* src, int n_src, void* blob, void* stream);
int ttsgen_bind_weights(ttsgen_handle* h, const void* blob);
/* Scratch of one call: one group of min(B, G) utterances (above); 0 when one utterance of T frames does not fit a group. */
size_t ttsgen_workspace_bytes(const ttsgen_handle* h, int B, int T);
/* Generator.forward (models.py:947-968): z [B, T, initial_channel] channel-last (the reference's x [B, C, T] transposed),
 * g NULL or [B, gin_channels] (the reference's g [B, gin, 1]); out [B, T * prod(up_rates)] (the reference's [B, 1, T']).
 * Frames are not masked (the reference's dec call has no mask): every frame of every utterance is computed.  Enqueues only -
 * no synchronisation, no host reads.  TTSDEC_ERR_DIMS when one utterance exceeds a group's bound. */
int ttsgen_forward(ttsgen_handle* h, const float* z, const float* g, int B, int T, float* out, void* workspace, size_t workspace_bytes,
                   void* stream);
/* Test aid: the same call stopped after n_stages upsampling stages (0 = after conv_pre).  B must fit one group.  The stage's
 * activated output - leaky_relu(x, 0.1), or 0.01 after the last stage - is left at the start of the workspace as
 * [B * T_s, C_s] fp32 (T_s = T * u_0 * ... * u_{n_stages-1}, C_s its channels; conv_pre: [B * T, C0]); nothing is written to out. */
int ttsgen_forward_stages(ttsgen_handle* h, const float* z, const float* g, int B, int T, int n_stages, void* workspace, size_t workspace_bytes,
                          void* stream);

/* The same forward with the arithmetic of its conv GEMMs as a call argument (as ttsdec_postnet has it): `precision` is
 * TTSDEC_PREC_F32 - then the call IS ttsgen_forward / ttsgen_forward_stages, the same code and the same bits, and `planes` is
 * ignored - or TTSDEC_PREC_SPLIT_F16 (opt-in: two fp16 planes per GEMM operand, three products, fp32 accumulate; held to the
 * exact path's parity bar); anything else is TTSDEC_ERR_INVALID_ARG.  These take a ttsgen_handle under the ttsvits_ prefix, as
 * ttsenc_style_* puts a second handle type under ttsenc_.
 *   Only GEMM operands are split.  x, the resblocks' running x', the branch sum and the bias / cond(g) / residual / sum /
 * division chain of the epilogues stay fp32, in the exact path's order; conv_post + tanh reads fp32.  Every conv input - z, and
 * the leaky-ReLU outputs between the convs - is held as planes (hi = fp16(x), lo = fp16((x - hi) * 2^11)); the split SATURATES:
 * an activation beyond +-65504 enters the next conv as +-65504, and there is no status word that says so (finite weights of a
 * trained generator keep activations orders of magnitude below it).
 *   A layer runs in split-fp16 when its input channels are a multiple of 8 and, where it is dilated, divide 64 or are a multiple
 * of 64 (the K tile of the split tiles); the resblocks of one stage switch together.  Any other layer keeps the exact fp32 tiles
 * inside a split-fp16 call (reading an fp32 copy of its input).  ModelConfig dims: every conv qualifies.  (ups[0] always does:
 * upsample_initial_channel is twice a multiple of 4.  So planes_bytes is never 0.)
 *   ttsvits_generator_planes_bytes: size of the second blob, the planes of the weights of every layer that runs in split-fp16 (per
 * weight of n elements: hi plane, lo plane, 4 n bytes rounded up to 256); 62.6 MB at the ModelConfig dims.  An fp32-only caller
 * allocates nothing.
 *   ttsvits_generator_pack_planes: builds them (256-byte aligned device memory) from the fp32 blob that is bound - a split of the
 * packed blob, in its layout (conv weights tap-major, ups as the polyphase 3-tap weight), not a second packing - on `stream`;
 * TTSDEC_ERR_NOT_BOUND when nothing is bound.  Call it again whenever the fp32 blob is repacked.
 *   ttsvits_generator_workspace_bytes(gen, TTSDEC_PREC_F32, B, T) == ttsgen_workspace_bytes(gen, B, T); split-fp16 adds the planes
 * of z ([G * T, initial_channel]) and, for a handle with both kinds of layer, one more activation buffer.  0 for a bad precision.
 *   ttsvits_generator_forward: z, g, B, T, out, workspace as ttsgen_forward; groups as there.  n_stages == n_up with out != NULL
 * is the full forward; 0 <= n_stages < n_up (out ignored), or n_stages == n_up with out == NULL, is ttsgen_forward_stages (B
 * must fit one group): whatever the precision, that stage's activated output is left as fp32 [B * T_s, C_s] at the start of
 * the workspace.  Any other n_stages is TTSDEC_ERR_INVALID_ARG.  Split-fp16 with
 * planes == NULL is TTSDEC_ERR_INVALID_ARG. */
size_t ttsvits_generator_planes_bytes(const ttsgen_handle* gen);
int ttsvits_generator_pack_planes(ttsgen_handle* gen, void* planes, void* stream);
size_t ttsvits_generator_workspace_bytes(const ttsgen_handle* gen, int precision, int B, int T);
int ttsvits_generator_forward(ttsgen_handle* gen, int precision, const void* planes, const float* z, const float* g, int B, int T,
                              int n_stages, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * VITS2 waveform discriminators: DiscriminatorP.forward and DiscriminatorS.forward, vits2/models.py:977-1083 (the members of
 * MultiPeriodDiscriminator, models.py:1086-1110).  Eval mode, exact fp32, inference only; weight norm only (spectral norm is not
 * built).  A second handle kind of the ttsvits_ family, as ttsenc_style_* is one of ttsenc_; it has no set_precision.
 *   period p > 0: DiscriminatorP(p, kernel_size, stride) - the waveform [B, T] reflect-padded on the right to a multiple of p and
 *     folded to [B, 1, H, p], H = ceil(T / p) (pad and fold are an index computation of the first layer); five (k, 1) convs
 *     1 -> 32 -> 128 -> 512 -> 1024 -> 1024 with strides (s, s, s, s, 1), padding (k - 1) / 2 and leaky_relu(0.1), then conv_post
 *     1024 -> 1 with 3 taps.
 *   period 0: DiscriminatorS - Conv1d 1 -> 16 (k 15), four grouped stride-4 k-41 convs 16 -> 64 -> 256 -> 1024 -> 1024 (4, 16, 64,
 *     256 groups), Conv1d 1024 -> 1024 (k 5), each with leaky_relu(0.1), then conv_post 1024 -> 1 (k 3); kernel_size and stride
 *     are ignored.
 * Activations are CHANNELS-LAST and PERIOD-MAJOR: feature map i is [B, p, H_i, C_i] (DiscriminatorS: p = 1, [B, L_i, C_i]), the
 * reference's [B, C_i, H_i, p] ([B, C_i, L_i]) permuted; H_{i+1} = (H_i + 2 pad - k) / stride + 1.  The dense convs (Ci >= 32, no
 * groups) are implicit GEMMs of the exact-fp32 tile with one fixed tile shape; layer 0, the grouped convs and conv_post are
 * direct kernels with a fixed summation order.  Nothing depends on B: a row gets the same bits alone and in any batch, and the
 * same call twice gives the same bits.
 * ------------------------------------------------------------------------------------- */
#define TTSVITS_DISC_MAX_CONVS 6
typedef struct ttsvits_disc_dims {
  int32_t period;      /* 0 = DiscriminatorS; else DiscriminatorP's period (2, 3, 5, 7, 11), 1..4096        */
  int32_t kernel_size; /* DiscriminatorP: 5; odd, 1..15                                                      */
  int32_t stride;      /* DiscriminatorP: 3; 1..16                                                           */
} ttsvits_disc_dims;
typedef struct ttsvits_disc_handle ttsvits_disc_handle;

/* Dimensions not built (an even or too large kernel_size, a stride or period out of range) are refused with TTSDEC_ERR_DIMS. */
int ttsvits_disc_create(const ttsvits_disc_dims* dims, ttsvits_disc_handle** out);
int ttsvits_disc_destroy(ttsvits_disc_handle* h);
const char* ttsvits_disc_last_hip_error(const ttsvits_disc_handle* h);
/* Source tensors for ttsvits_disc_pack_weights (device fp32, the reference's parameter shapes, EFFECTIVE weights - g * v / ||v||
 * of weight_norm folded), in this order: convs.i.weight, convs.i.bias for every conv i, then conv_post.weight, conv_post.bias
 * (12 tensors for DiscriminatorP, 14 for DiscriminatorS).  None may be NULL. */
int ttsvits_disc_num_weight_tensors(const ttsvits_disc_handle* h);
size_t ttsvits_disc_packed_bytes(const ttsvits_disc_handle* h);
int ttsvits_disc_pack_weights(ttsvits_disc_handle* h, const float* const* src, int n_src, void* blob, void* stream);
int ttsvits_disc_bind_weights(ttsvits_disc_handle* h, const void* blob);
/* Scratch of a scores-only call (fmaps == NULL): two buffers that the layers' outputs alternate between.  0 when the call is
 * refused: B or T <= 0; a T the reference's reflect pad itself refuses (T % p != 0 and p - T % p >= T); or B * T or an
 * activation's element count beyond 2^31 - 1 (32-bit row and element indices; split the batch). */
size_t ttsvits_disc_workspace_bytes(const ttsvits_disc_handle* h, int B, int T);
/* forward (models.py:1034-1053 / 1072-1083): y [B, T] (the reference's [B, 1, T]) -> scores [B, H_last * p] in the reference's
 * flatten order (index h * p + w) - the same memory as its last feature map [B, 1, H_last, p].
 *   fmaps: NULL, or num_convs (5 / 6) device pointers, 16-byte aligned, that receive the activated output of every conv in the
 * layout above; the workspace is then not used and may be NULL.  With fmaps == NULL the activations stay in the workspace
 * (256-byte aligned, at least ttsvits_disc_workspace_bytes).
 * TTSDEC_ERR_DIMS for a call the size function refuses.  Enqueues only - no synchronisation, no host reads. */
int ttsvits_disc_forward(ttsvits_disc_handle* h, const float* y, int B, int T, float* scores, float* const* fmaps, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * VITS2 duration discriminators: DurationDiscriminatorV1 and DurationDiscriminatorV2, vits2/models.py:183-329 (the net_dur_disc of
 * the reference's train.py, its DUR_*.pth checkpoint).  Eval mode, exact fp32, inference only.  A third handle kind of the
 * ttsvits_ family; it has no set_precision.  C = in_channels, F = filter_channels, every conv has 3 taps and padding 1; neither
 * class uses gin_channels / g.  Activations are CHANNEL-LAST, one row per token: x [B, T, C] as ttsvits_text_encoder writes it.
 *   trunk (once per call):          V2: h = norm_2(relu(conv_2(norm_1(relu(conv_1(x m))) m)));  V1: h = conv_2(conv_1(x m) m)
 *   probability (per duration):     u = pre_out_conv_1(cat([h, dur_proj(dur)], 1) m)  [V2: u = pre_out_norm_1(relu(u))]
 *                                   u = pre_out_conv_2(u m)                           [V2: u = pre_out_norm_2(relu(u))]
 *                                   p = sigmoid(output_layer(u m))   - sigmoid(output_layer's bias) at a masked token
 * m is the token mask t < lengths[b], applied as a SELECT: what x, hidden and dur hold at masked tokens is never read into a
 * result.  The four wide convs (conv_1, conv_2, the h half of pre_out_conv_1, pre_out_conv_2) are implicit GEMMs of the exact-fp32
 * tile with one fixed tile shape.  cat([h, d]) is never built: dur_proj is rank one, so its half of pre_out_conv_1 is folded at
 * pack time into a slope and an offset table [3][F] (S[tap][n] = sum_c W[n, F + c, tap] w_dur[c], O with b_dur; c ascending), and
 * the h half is computed once per call for all its durations.  Nothing depends on B: an utterance in a padded batch gets bit for
 * bit what it gets alone at T = its own length, n_dur = 2 gives the bits of two n_dur = 1 calls, and the same call twice gives the
 * same bits (no atomics).
 * ------------------------------------------------------------------------------------- */
#define TTSVITS_DURDISC_MAX_CHANNELS 1024
typedef struct ttsvits_durdisc_dims {
  int32_t version;         /* 1 = DurationDiscriminatorV1, 2 = DurationDiscriminatorV2                                  */
  int32_t in_channels;     /* the text encoder's hidden_channels (192); a multiple of 4, <= TTSVITS_DURDISC_MAX_CHANNELS */
  int32_t filter_channels; /* 192 or 256 in the reference's configurations; a multiple of 4, <= the same cap            */
  int32_t kernel_size;     /* 3                                                                                        */
} ttsvits_durdisc_dims;
typedef struct ttsvits_durdisc_handle ttsvits_durdisc_handle;

/* TTSDEC_ERR_DIMS - never another computation - for a version other than 1 or 2, a kernel_size other than 3, and channel counts
 * that are not positive multiples of 4 or exceed the cap. */
int ttsvits_durdisc_create(const ttsvits_durdisc_dims* dims, ttsvits_durdisc_handle** out);
int ttsvits_durdisc_destroy(ttsvits_durdisc_handle* h);
const char* ttsvits_durdisc_last_hip_error(const ttsvits_durdisc_handle* h);
/* Source tensors for ttsvits_durdisc_pack_weights (device fp32, the reference's parameter shapes), in this order - the state
 * dict's, the [V2] pairs only for version 2 and V1's unused pre_out_norm_* left out: conv_1.weight [F, C, 3], conv_1.bias,
 * [V2: norm_1.gamma, norm_1.beta,] conv_2.weight [F, F, 3], conv_2.bias, [V2: norm_2.gamma, norm_2.beta,] dur_proj.weight [F, 1, 1],
 * dur_proj.bias, pre_out_conv_1.weight [F, 2F, 3], pre_out_conv_1.bias, [V2: pre_out_norm_1.gamma, .beta,] pre_out_conv_2.weight
 * [F, F, 3], pre_out_conv_2.bias, [V2: pre_out_norm_2.gamma, .beta,] output_layer.0.weight [1, F], output_layer.0.bias [1]:
 * 12 tensors for V1, 20 for V2.  None may be NULL. */
int ttsvits_durdisc_num_weight_tensors(const ttsvits_durdisc_handle* h);
size_t ttsvits_durdisc_packed_bytes(const ttsvits_durdisc_handle* h);
int ttsvits_durdisc_pack_weights(ttsvits_durdisc_handle* h, const float* const* src, int n_src, void* blob, void* stream);
int ttsvits_durdisc_bind_weights(ttsvits_durdisc_handle* h, const void* blob);
/* Scratch of either call with n_dur (1 or 2) durations (the trunk's is that of n_dur = 1): a multiple of 256, monotone in B, T
 * and n_dur; 0 for a NULL handle, a size <= 0, n_dur outside {1, 2} or n_dur * B * T > INT32_MAX / 4096 rows (the GEMM core counts
 * rows and offsets in 32 bits; split the batch). */
size_t ttsvits_durdisc_workspace_bytes(const ttsvits_durdisc_handle* h, int B, int T, int n_dur);
/* forward up to the loop over the durations (models.py:243-250 / 317-322): x [B, T, C], lengths [B] int32 (device) -> hidden_out
 * [B, T, F] = h * m (zero at masked tokens, where the reference's own h is never read).  x and hidden_out 16-byte aligned.
 * Both calls: TTSDEC_ERR_INVALID_ARG for a NULL or misaligned pointer, B or T <= 0, n_dur outside {1, 2}, or a workspace that is
 * NULL, not 256-byte aligned or smaller than ttsvits_durdisc_workspace_bytes; TTSDEC_ERR_NOT_BOUND before bind_weights;
 * TTSDEC_ERR_DIMS for a call the size function refuses.  Enqueue only - no synchronisation, no host reads. */
int ttsvits_durdisc_trunk(ttsvits_durdisc_handle* h, const float* x, const int32_t* lengths, int B, int T, float* hidden_out, void* workspace,
                          size_t workspace_bytes, void* stream);
/* forward_probability (models.py:222-236 / 298-310) for n_dur durations at once: hidden [B, T, F] (16-byte aligned; the trunk's
 * output, or the reference's h - it is masked again here), dur [n_dur, B, T] -> prob_out [n_dur, B, T] (the reference's [B, T, 1]
 * per duration) and, unless logit_out is NULL, the pre-sigmoid logits in the same shape. */
int ttsvits_durdisc_prob(ttsvits_durdisc_handle* h, const float* hidden, const int32_t* lengths, const float* dur, int n_dur, int B, int T,
                         float* prob_out, float* logit_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * VITS2 duration likelihood: StochasticDurationPredictor.forward(x, x_mask, w, g=g), vits2/models.py:78-125 - the `l_length` of
 * SynthesizerTrn.forward (:1258-1259) before its division, the VL/dur of the reference's validation.  Eval mode, exact fp32,
 * inference only.  A fourth handle kind of the ttsvits_ family; it has no set_precision.  C = in_channels; activations are
 * CHANNEL-LAST, x [B, T, C] as ttsvits_text_encoder writes it; m is the token mask t < lengths[b], applied as a select.
 *   x' = proj(convs(pre(x) [+ cond(g)])) m;  g_q = x' + post_proj(post_convs(post_pre(w))) m
 *   z_q = e_q m -> post_flows: ElementwiseAffine, 4 x (ConvFlow conditioned on g_q, Flip);  (z_u, z1) = z_q
 *   u = sigmoid(z_u) m, z0 = (w - u) m;  logdet_tot_q = the posterior flows' log-dets + sum (logsigmoid(z_u) + logsigmoid(-z_u)) m
 *   z = flows(cat([Log(z0), z1])): ElementwiseAffine, n_flows x (ConvFlow conditioned on x', Flip);  logdet_tot = Log's and theirs
 *   nll = sum 0.5 (log 2pi + z^2) m - logdet_tot  +  sum -0.5 (log 2pi + e_q^2) m - logdet_tot_q
 * The kernels are those of ttsdur_sdp_reverse (one launch per DDSConv layer over tiles of 16 tokens) with the spline's forward
 * branch (transforms.py:100-209, searchsorted on cumwidths, linear tails) and the elementwise steps in their epilogues.  Every
 * token row keeps its own log-det sums; one last launch sums an utterance's tokens in a fixed order and adds the Gaussian terms:
 * no atomics, an utterance in a padded batch gets bit for bit what it gets alone at T = its own length, and the same call twice
 * gives the same bits.
 * ------------------------------------------------------------------------------------- */
typedef struct ttsvits_durnll_dims {
  int32_t in_channels;  /* hidden_channels (192): width of x and of the predictor (models.py:40); a multiple of 4, <= 256 */
  int32_t kernel_size;  /* 3 (the only size built)                                                                       */
  int32_t n_flows;      /* 4 (2..8)                                                                                      */
  int32_t gin_channels; /* 0, or the width of the speaker vector g (cond, 1x1)                                           */
} ttsvits_durnll_dims;
typedef struct ttsvits_durnll_handle ttsvits_durnll_handle;

/* TTSDEC_ERR_DIMS for what ttsdur_create refuses of a kind-0 predictor: kernel_size != 3, in_channels not a multiple of 4 or
 * above 256, n_flows < 2 or > 8, gin_channels < 0. */
int ttsvits_durnll_create(const ttsvits_durnll_dims* dims, ttsvits_durnll_handle** out);
int ttsvits_durnll_destroy(ttsvits_durnll_handle* h);
const char* ttsvits_durnll_last_hip_error(const ttsvits_durnll_handle* h);
/* Source tensors for ttsvits_durnll_pack_weights (device fp32, the reference's parameter shapes), in this order - a blob of its
 * own, every parameter of the module (a trunk is the 28 tensors pre.weight, pre.bias, the DDSConv's 24, proj.weight, proj.bias as
 * ttsdur_pack_weights lists them; a ConvFlow the same 28 with pre [C, 1, 1] and proj [29, C, 1]):
 *   pre, convs, proj (28);  flows.0.m, flows.0.logs [2, 1];  flows.{2k+1} for k = 0 .. n_flows-1 (28 each; flows.1 included);
 *   post_pre [C, 1, 1], post_convs, post_proj (28);  post_flows.0.m, post_flows.0.logs;  post_flows.{1, 3, 5, 7} (28 each);
 *   when gin_channels > 0: cond.weight [C, gin, 1], cond.bias [C].
 * 172 + 28 n_flows tensors (284 at n_flows = 4), 2 more with g.  None may be NULL. */
int ttsvits_durnll_num_weight_tensors(const ttsvits_durnll_handle* h);
size_t ttsvits_durnll_packed_bytes(const ttsvits_durnll_handle* h);
int ttsvits_durnll_pack_weights(ttsvits_durnll_handle* h, const float* const* src, int n_src, void* blob, void* stream);
int ttsvits_durnll_bind_weights(ttsvits_durnll_handle* h, const void* blob);
/* Scratch of one ttsvits_durnll_forward call of B utterances of T tokens; 0 for a NULL handle or a size <= 0. */
size_t ttsvits_durnll_workspace_bytes(const ttsvits_durnll_handle* h, int B, int T);
/* x [B, T, C], lengths [B] int32 (device), g NULL or [B, gin], w [B, T] the durations (the reference's [B, 1, T]), noise [B, 2, T]
 * the reference's draw torch.randn(B, 2, T) (e_q before its mask) -> nll_out [B]; unless NULL, terms_out [B, 4] = { sum -0.5
 * (log 2pi + e_q^2) m, logdet_tot_q, sum 0.5 (log 2pi + z^2) m, logdet_tot } with nll = (terms[2] - terms[3]) + (terms[0] -
 * terms[1]), and z_out [B, 2, T] = z after the last flow (zero at masked tokens).  TTSDEC_ERR_INVALID_ARG for a NULL x, lengths, w,
 * noise or nll_out, B or T <= 0, or g with gin_channels = 0; TTSDEC_ERR_NOT_BOUND before bind_weights; TTSDEC_ERR_DIMS for
 * B * T > 2^30; TTSDEC_ERR_WORKSPACE for a workspace that is not 256-byte aligned or smaller than
 * ttsvits_durnll_workspace_bytes.  Enqueue only - no synchronisation, no host reads. */
int ttsvits_durnll_forward(ttsvits_durnll_handle* h, const float* x, const int32_t* lengths, const float* g, const float* w, const float* noise,
                           int B, int T, float* nll_out, float* terms_out, float* z_out, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ---------------------------------------------------------------------------------------
 * VITS2 duration predictors and length regulation: the `self.dp(...)` and the prior expansion of SynthesizerTrn.infer,
 * vits2/models.py:1288-1320.  Eval mode, exact fp32 (fp32 vector ALU throughout).  Activations are CHANNEL-LAST: the text
 * encoder's x [B, T, C], m / logs [B, T, inter] feed in as ttsvits_text_encoder writes them.
 *   kind 0, StochasticDurationPredictor reverse (models.py:29-137): conditioning x' = proj(DDSConv(pre(x) [+ cond(g)])) * mask;
 *     z = noise * noise_scale; the flows [Flip, ConvFlow_n, Flip, ..., ConvFlow_2, Flip, ElementwiseAffine] (flows.1 is dropped,
 *     :127-128) with ConvFlow reverse = pre (1 -> C) on x0, DDSConv(+ x'), proj (C -> 29) * mask, the inverse rational-quadratic
 *     spline (transforms.py:50-209, linear tails at +-5) on x1; logw = channel 0.
 *   kind 1, DurationPredictor (models.py:140-180): (x [+ cond(g)]) -> conv k3 on x * mask, ReLU, LayerNorm, twice -> proj (F -> 1)
 *     on x * mask, * mask.
 * DDSConv layer i (modules.py:84-127, dilation 3^i): one launch per layer over tiles of 16 frames: the depthwise conv (zero
 * padding per utterance), LayerNorm, GELU (erf), the 1x1 C x C conv, LayerNorm, GELU and the residual.  A ConvFlow's pre and
 * `+ g` ride in its first layer's load; proj, the spline, Flip and ElementwiseAffine in its last layer's epilogue.
 * Frames at or beyond lengths[b] are masked as the reference masks them; the outputs there are 0.
 * ------------------------------------------------------------------------------------- */
typedef struct ttsdur_dims {
  int32_t kind;             /* 0 = StochasticDurationPredictor (reverse only), 1 = DurationPredictor                     */
  int32_t in_channels;      /* hidden_channels (192): width of x; the SDP's width everywhere (models.py:40)               */
  int32_t filter_channels;  /* DurationPredictor: 256 (SynthesizerTrn); ignored by kind 0                                */
  int32_t kernel_size;      /* 3 (the only size built)                                                                   */
  int32_t n_flows;          /* kind 0: 4 (2..8); ignored by kind 1                                                       */
  int32_t gin_channels;     /* 0, or the width of the speaker vector g (cond, 1x1)                                       */
} ttsdur_dims;
typedef struct ttsdur_handle ttsdur_handle;

/* Dimensions not built (kernel_size != 3, channels not multiples of 4 or above 256, n_flows < 2 or > 8) are refused with
 * TTSDEC_ERR_DIMS. */
int ttsdur_create(const ttsdur_dims* dims, ttsdur_handle** out);
int ttsdur_destroy(ttsdur_handle* h);
const char* ttsdur_last_hip_error(const ttsdur_handle* h);
/* Source tensors for ttsdur_pack_weights (device fp32, the reference's parameter shapes), in this order (C = in_channels):
 *  kind 0:  pre.weight [C, C, 1], pre.bias [C];
 *           convs (DDSConv), per layer i in 0..2: convs_sep.i.weight [C, 1, 3], convs_sep.i.bias [C], convs_1x1.i.weight
 *               [C, C, 1], convs_1x1.i.bias [C], norms_1.i.gamma, norms_1.i.beta, norms_2.i.gamma, norms_2.i.beta   (8 per layer);
 *           proj.weight [C, C, 1], proj.bias [C];  flows.0.m [2, 1], flows.0.logs [2, 1];
 *           per ConvFlow flows.{2k+1}, k = 1 .. n_flows-1 (flows.1 is unused by reverse and not passed): pre.weight [C, 1, 1],
 *               pre.bias [C], its DDSConv's 24 tensors as above, proj.weight [29, C, 1], proj.bias [29];
 *           when gin_channels > 0: cond.weight [C, gin, 1], cond.bias [C].          (114 tensors at n_flows = 4 without g)
 *  kind 1:  conv_1.weight [F, C, 3], conv_1.bias [F], norm_1.gamma, norm_1.beta [F], conv_2.weight [F, F, 3], conv_2.bias,
 *           norm_2.gamma, norm_2.beta, proj.weight [1, F, 1], proj.bias [1];
 *           when gin_channels > 0: cond.weight [C, gin, 1], cond.bias [C].          (10 tensors without g) */
int ttsdur_num_weight_tensors(const ttsdur_handle* h);
size_t ttsdur_packed_bytes(const ttsdur_handle* h);
int ttsdur_pack_weights(ttsdur_handle* h, const float* const* src, int n_src, void* blob, void* stream);
int ttsdur_bind_weights(ttsdur_handle* h, const void* blob);
/* Scratch of one ttsdur_sdp_reverse / ttsdur_dp_forward call of B utterances of T tokens. */
size_t ttsdur_workspace_bytes(const ttsdur_handle* h, int B, int T);
/* StochasticDurationPredictor.forward(x, x_mask, g=g, reverse=True, noise_scale) (kind 0): x [B, T, C] channel-last,
 * lengths [B] int32 device (x_mask = t < lengths[b]), g NULL or [B, gin], noise [B, 2, T] (the reference's torch.randn(B, 2, T),
 * channel-first, before the noise_scale factor); logw out [B, T] (the reference's [B, 1, T]).  Enqueues only. */
int ttsdur_sdp_reverse(ttsdur_handle* h, const float* x, const int32_t* lengths, const float* g, const float* noise, float noise_scale,
                       int B, int T, float* logw, void* workspace, size_t workspace_bytes, void* stream);
/* DurationPredictor.forward(x, x_mask, g) (kind 1): the same tensors, no noise. */
int ttsdur_dp_forward(ttsdur_handle* h, const float* x, const int32_t* lengths, const float* g, int B, int T, float* logw,
                      void* workspace, size_t workspace_bytes, void* stream);
/* Length regulation, first half (models.py:1304-1306): w = exp(logw) * mask * length_scale, w_ceil = ceil(w);
 * cum [B, T] int32 = the running sum of w_ceil over an utterance's tokens (padded tokens add w_ceil = 0 as in the reference),
 * y_len [B] int32 = max(1, sum w_ceil); status [2] int32 = { max_b y_len, flags }: flag 1 = a non-finite w, flag 2 = a sum beyond
 * 2^24 frames (where fp32 stops counting exactly; cum / y_len are then meaningless).  One workgroup; the caller reads status
 * once (the reference's host sync for T_y = max y_len) and must not call ttsdur_expand when flags != 0. */
int ttsdur_lengths(ttsdur_handle* h, const float* logw, const int32_t* lengths, float length_scale, int B, int T, int32_t* cum,
                   int32_t* y_len, int32_t* status, void* stream);
/* Length regulation, second half (models.py:1307-1320 without the dense path matmul): for frame t < T_y of utterance b,
 * token j with cum[j-1] <= t < cum[j] (none when t >= cum[T-1]):  m_p[b, t, :] = m[b, j, :], logs_p[b, t, :] = logs[b, j, :]
 * (zeros without a token), z_p[b, t, c] = m_p + eps[b, c, t] * exp(logs_p) * noise_scale, channel-last [B, T_y, inter]
 * (the flow's input layout); attn [B, T_y, T] = 1 at (t, j), else 0 (NULL: not written).  eps [B, inter, eps_T] is the
 * reference's torch.randn_like(m_p) with eps_T >= T_y frames per channel row.  m, logs [B, T, inter] channel-last. */
int ttsdur_expand(ttsdur_handle* h, const int32_t* cum, const float* m, const float* logs, const float* eps, int eps_T, float noise_scale,
                  int B, int T, int inter, int T_y, float* z_p, float* m_p, float* logs_p, float* attn, void* stream);

/* ---------------------------------------------------------------------------------------
 * VITS2 posterior encoder: PosteriorEncoder.forward, vits2/models.py:858-897 - the `self.enc_q(y, y_lengths, g=g_src)` of
 * SynthesizerTrn.voice_conversion, models.py:1333.  Eval mode, dilation_rate 1 (the ModelConfig's), g constant over time.
 *   x_mask = sequence_mask(lengths, T);  x = pre(y) * x_mask (1x1, spec -> hidden);  x = WN(x, x_mask, g) (modules.py:185-210,
 *   n_layers layers of a kernel_size-tap hidden -> 2 hidden conv, the gate [+ cond_layer(g)], a 1x1 res/skip conv);
 *   stats = proj(x) * x_mask (1x1, hidden -> 2 inter);  m, logs = split(stats);  z = (m + eps * exp(logs)) * x_mask.
 * The spectrogram comes in as the reference receives it, channel-first [B, spec, T]; one staging kernel writes the channel-last
 * GEMM operand (channels zero-padded to a multiple of 8, so any spec width works - 513 for a linear-spectrogram posterior).
 * Every conv runs on the library's GEMM core (ttspost_set_precision), the WN loop is the flow's (ttsvits_flow_*).  Outputs are
 * CHANNEL-LAST [B, T, inter]; padded frames are zero.
 * ------------------------------------------------------------------------------------- */
typedef struct ttspost_dims {
  int32_t spec_channels;    /* 80 (mel posterior) or 513 (linear spectrogram, n_fft 1024): channels of y, 1..4096        */
  int32_t inter_channels;   /* 192: channels of z, m and logs (proj emits 2 inter); a multiple of 4                       */
  int32_t hidden_channels;  /* 192: WN width; a multiple of 4                                                             */
  int32_t kernel_size;      /* 5: WN conv taps (odd)                                                                      */
  int32_t n_layers;         /* 16: WN layers, 1..32                                                                       */
  int32_t gin_channels;     /* 0, or the speaker-embedding width of WN.cond_layer (a multiple of 4, <= 4096)              */
} ttspost_dims;
typedef struct ttspost_handle ttspost_handle;

/* Dimensions outside the ranges above are refused with TTSDEC_ERR_DIMS. */
int ttspost_create(const ttspost_dims* dims, ttspost_handle** out);
int ttspost_destroy(ttspost_handle* h);
const char* ttspost_last_hip_error(const ttspost_handle* h);
/* TTSDEC_PREC_F32 (default, exact fp32 matrix instruction) or TTSDEC_PREC_SPLIT_F16 (hi + lo fp16 planes, fp32 accumulate), as
 * ttsvits_set_precision; the elementwise math is fp32 in both. */
int ttspost_set_precision(ttspost_handle* h, int precision);
int ttspost_get_precision(const ttspost_handle* h);
/* Source tensors for ttspost_pack_weights (device fp32, the reference's parameter shapes), in this order:
 *   pre.weight [hidden, spec, 1], pre.bias [hidden];
 *   when gin_channels > 0: enc.cond_layer EFFECTIVE weight (g * v / ||v||) [2 hidden n_layers, gin, 1], bias;
 *   per WN layer j: enc.in_layers.j effective weight [2 hidden, hidden, k], bias, enc.res_skip_layers.j effective weight
 *       [2 hidden (hidden for the last layer), hidden, 1], bias;
 *   proj.weight [2 inter, hidden, 1], proj.bias [2 inter].
 * (4 + 4 n_layers tensors, + 2 with gin_channels > 0: 70 at the ModelConfig dims with a speaker embedding.) */
int ttspost_num_weight_tensors(const ttspost_handle* h);
size_t ttspost_packed_bytes(const ttspost_handle* h);
int ttspost_pack_weights(ttspost_handle* h, const float* const* src, int n_src, void* blob, void* stream);
int ttspost_bind_weights(ttspost_handle* h, const void* blob);
/* Scratch of one ttspost_forward call of B utterances of T frames (256-byte aligned). */
size_t ttspost_workspace_bytes(const ttspost_handle* h, int B, int T);
/* y [B, spec, T] channel-first fp32 (device), lengths [B] int32 (device), g NULL or [B, gin_channels] (the reference's g [B, gin, 1];
 * TTSDEC_ERR_INVALID_ARG on a handle with gin_channels == 0), eps [B, inter, eps_T] channel-first with eps_T >= T (the reference's
 * torch.randn_like(m), read as ttsdur_expand reads its eps).  z, m, logs out [B, T, inter] channel-last.  Enqueues only. */
int ttspost_forward(ttspost_handle* h, const float* y, const int32_t* lengths, const float* g, const float* eps, int eps_T, int B, int T,
                    float* z, float* m, float* logs, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TTSDEC_H */
