/*
 * aprilx_engine.h -- engine-level C ABI of libaprilasr.so (MI355X build).
 *
 * The reference runs its networks through ONNXRuntime's C API behind
 * src/ort_util.{h,c}: one g_ort->Run per graph per session per chunk, batch 1
 * (src/april_session.c:145,160,176).  This header is the batched replacement of
 * that inner boundary plus the few knobs a multi-session / multi-GPU host needs.
 * Plain pointers and sizes only; every function cites what it replaces.
 *
 * All functions are safe to call from any thread; sessions must not be fed from
 * two threads at once (same rule as the reference).
 */
#ifndef APRILX_ENGINE_H
#define APRILX_ENGINE_H
#include "april_api.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Dimensions read from the model's graphs (reference src/april_model.h:35-41). */
typedef struct AprilxDims {
    int32_t n_layers, d_model, hidden, ffn, joiner, vocab, mel, seg, seg_step, context;
    int32_t fft_size, frame_shift, sample_rate, blank_id, n_devices;
    int32_t precision;          /* 0: fp32 GEMMs (default); 1: fp16 operands, fp32 accumulate (env APRIL_PRECISION=f16) */
    int32_t d_model_file;       /* 0, or the model file's d_model when its layer widths (any that are not multiples of 64) were rounded up to multiples of
                                   64 at load: d_model, hidden, ffn, joiner above are then the padded widths the engine runs */
    int64_t param_count;
} AprilxDims;
APRIL_EXPORT int aprilx_model_dims(AprilASRModel model, AprilxDims *out);
/* token text by id (reference src/params.c:31-33 get_token) */
APRIL_EXPORT const char *aprilx_model_token(AprilASRModel model, int32_t id);

/* ---- weight distribution (multi-GPU) -------------------------------------------------------
 * Sessions are independent, so a node's session pool is partitioned across its GPUs and the only
 * collective is the broadcast of the packed weights at model load (reference load site
 * src/april_model.c:57-61; the reference has no multi-device path).  The library does it with RCCL:
 *   - one process, several GPUs: aam_create_model with APRIL_GPU_DEVICES=0,1,... uploads the weights
 *     once and broadcasts them to the other devices (ncclCommInitAll + grouped ncclBroadcast);
 *   - one process per GPU: rank 0 parses the .april file (aam_create_model), calls
 *     aprilx_broadcast_get_id and hands the 128 bytes to the other ranks by any means (a launcher's
 *     store, a file, torch.distributed); then EVERY rank calls aprilx_model_broadcast.  Rank 0 passes
 *     its model and gets it back; the others pass NULL and receive a model built from the metadata and
 *     the weights that arrive in their GPU's memory over xGMI -- no file access, no host staging.
 * The blob functions below carry the same content through host memory (machines without RCCL peers,
 * the gloo test path, the on-disk cache).                                                      */
typedef struct AprilxLoadInfo {
    double broadcast_ms;        /* wall time of the weight broadcast (0 if none happened) */
    double comm_init_ms;        /* wall time of the RCCL communicator set-up */
    uint64_t broadcast_bytes;
    int32_t ranks;              /* devices / processes the weights were broadcast to, including the root */
    int32_t used_rccl;
} AprilxLoadInfo;
/* writes an RCCL unique id (128 bytes) to id_out; returns its size, -1 on failure */
APRIL_EXPORT int aprilx_broadcast_get_id(void *id_out, size_t cap);
APRIL_EXPORT AprilASRModel aprilx_model_broadcast(AprilASRModel root_model, int rank, int world, const void *id_bytes);
APRIL_EXPORT int aprilx_model_load_info(AprilASRModel model, AprilxLoadInfo *out);
APRIL_EXPORT size_t aprilx_model_blob_size(AprilASRModel model);
APRIL_EXPORT int aprilx_model_export_blob(AprilASRModel model, void *dst, size_t dst_size);
/* `blob` may be a host pointer or a device pointer on the calling process's GPU */
APRIL_EXPORT AprilASRModel aprilx_model_from_blob(const void *blob, size_t size, int blob_is_device_ptr);
/* The same blob as a file next to the model: a cache of the parsed + MFMA-packed weights, so that later loads skip the
 * ONNX parse and the packing (the reference re-parses the .april file at every
 * aam_create_model, april_model.c:24-107).  save returns 0 on success; load returns NULL on any failure. */
APRIL_EXPORT int aprilx_model_save_blob(AprilASRModel model, const char *path);
/* fp16 variant of the cache file for fp16-operand mode (BASELINE configs[4]): the MFMA-packed matrices as binary16, half the
 * size; aprilx_model_load_blob recognises it and requires APRIL_PRECISION=f16 on a GPU runtime */
APRIL_EXPORT int aprilx_model_save_blob_f16(AprilASRModel model, const char *path);
APRIL_EXPORT AprilASRModel aprilx_model_load_blob(const char *path);

/* ---- batched session driving ------------------------------------------------------------
 * aas_feed_pcm16 / aas_flush (reference april_api.h:183,186) for n sessions in ONE call, so
 * that all of them advance in the same GPU steps.  Blocks until the work is done; handlers
 * of synchronous sessions run on the calling thread before it returns.                    */
APRIL_EXPORT void aprilx_feed_many(size_t n, AprilASRSession *sessions, const short *const *pcm16, const size_t *short_counts);
APRIL_EXPORT void aprilx_flush_many(size_t n, AprilASRSession *sessions);
/* block until an asynchronous session has consumed everything queued so far */
APRIL_EXPORT void aprilx_session_drain(AprilASRSession session);
/* Pipelined group feed: queue one feed for each of the n sessions (the samples are COPIED, as for an asynchronous session,
 * reference src/april_session.c:479-500), then block only until every session has at most `depth - 1` feeds that are
 * queued or in progress.  depth = 2 is double buffering: the call for feed k + 1 returns when feed k is complete, so the
 * library prepares and launches feed k + 1 while the GPU still works on feed k.  depth = 1 waits for this very feed
 * (aprilx_feed_many without lending the buffers).  Results arrive in feed order: handlers of synchronous sessions run on the
 * calling thread before the call returns (for the feeds that have completed by then), those of asynchronous sessions on the
 * library thread.  aprilx_drain_many waits for everything queued and delivers what is left.                              */
APRIL_EXPORT void aprilx_feed_many_pipelined(size_t n, AprilASRSession *sessions, const short *const *pcm16, const size_t *short_counts, int depth);
APRIL_EXPORT void aprilx_drain_many(size_t n, AprilASRSession *sessions);

/* ---- direct network evaluation (parity tests) -------------------------------------------
 * Same tensors as the three ORT Run calls, with a leading batch of n independent sessions:
 *   encoder: x[n][seg][mel], h[n][L][d_model], c[n][L][hidden] -> eout[n][joiner], h2, c2
 *            (reference src/april_session.c:131-148)
 *   decoder: context[n][2] int64 -> dout[n][joiner]              (:151-163)
 *   joiner : eout[n][joiner], dout[n][joiner] -> logits[n][vocab] (:166-179)
 *   fbank  : n frames of fft_size PCM16 samples -> n rows of `mel` log energies
 *            (reference src/fbank.c:228-296 per frame)
 * These use state slots 0..n-1 directly and must not be mixed with live sessions.        */
APRIL_EXPORT int aprilx_run_encoder(AprilASRModel model, int n, const float *x, const float *h, const float *c,
                                    float *eout, float *h2, float *c2);
APRIL_EXPORT int aprilx_run_decoder(AprilASRModel model, int n, const int64_t *context, float *dout);
APRIL_EXPORT int aprilx_run_joiner(AprilASRModel model, int n, const float *eout, const float *dout, float *logits);
APRIL_EXPORT int aprilx_run_fbank(AprilASRModel model, int n_frames, const int16_t *pcm_frames, float *out);
/* The device's copy of the search decision (reference src/april_session.c:306-429, the part the next network call depends
 * on) in isolation: op 0 = one joiner round for n rows with GIVEN logits[n][vocab], session times now_ms[n] and search states
 * state_io[n][4] = {context[0], context[1], last active token or -1, time of the last emission in ms}; writes the 16-byte
 * records {idx, max, blank logit, flags: 1 valid | 2 blank | 4 context changed} to records_out[n][4 x 32 bit] and the new states
 * to state_io.  op 1 = the end-of-flush reset (:561-563: tokens forgotten, context cleared unless it starts with blank).
 * Tests only (uses slots 0..n-1; must not be mixed with live sessions). */
APRIL_EXPORT int aprilx_run_decide(AprilASRModel model, int n, int op, const float *logits, float early_emit, const int32_t *now_ms,
                                   int round, int32_t *state_io, void *records_out);

/* The host-side plan of a row-epilogue GEMM out[M, N] = A[M, K] x W (K in `kz` slabs; `zcount` same-shape problems per launch;
 * tile_ok 0 = round-2 schedules, 1 = GM_TILE by the occupancy rule, 2 = GM_TILE always (fp16 tile path); force = the caller
 * needs the fused form): out[0] = 1 when the plan keeps all of K in the workgroup (row epilogue fused into the GEMM), out[1] =
 * partial planes the split form writes (finished by the row kernel), out[2] = 1 when the occupancy rule picks GM_TILE.  No GPU
 * needed; tests only (the engine and the launch wrappers plan with the same function, csrc/gemm_plan.h). */
APRIL_EXPORT int aprilx_plan_gemm(int M, int N, int kz, int zcount, int tile_ok, int force, int32_t *out);
/* The plan of one GEMM argument block as the launch wrappers see it (csrc/kernels.h gemm_plan).  in[22]: M N K K0 K1 kz epi a_op wt
 * wave_mask p_add? x_scale? zcount tile_ok force_fullk lda0 x_scale.groups r_scale.groups (0: none) out? out16? state16? ssq_out?
 * out[13]: the capabilities found for it (stream-kernel form, GM_KW, GM_PP, 192-column GM_PP), then route form mode mt nt zs planes
 * fused error (csrc/gemm_plan.h).  No GPU needed; tests only. */
APRIL_EXPORT int aprilx_gemm_plan_debug(const int32_t *in, int32_t *out);
/* ONE GEMM launch of csrc/kernels.h against host arrays, the way the engine launches it (csrc/gemm_debug_api.cc; needs a GPU, no
 * model; tests only: tests/gemm_ref.py states the mathematics it is compared with).  n = 1..3 problems of one shape.
 * desc[48], int32: 0 n, 1 M, 2 N, 3 K, 4 K0, 5 K1, 6 kz, 7 epi, 8 a_op, 9 wt, 10 wave_mask, 11 tile_ok, 12 force_fullk, 13 hidden,
 *   14 ldo, 15 lda0, 16 lda1, 17 ldr, 18 ld_state, 19 ldp, 20 value of the run_flag word (-1: no run_flag), 21 run_gen, 22 ctx_vocab,
 *   23 same_idx_b, 24 rows_alloc (rows of every row-indexed device array; >= M rounded up to 256), 25 slots (rows of the slot tables),
 *   26 a0 rows, 27 a1 rows, 28 a0b rows, 29 x_scale.groups, 30 r_scale.groups, 31 out != null, 32 out16 != null, 33 state16 != null,
 *   34..36 gemm_tile_pin(enable, mt, zs), 37..38 gemm_kw_pin(enable, mt), 39..40 gemm_pp_pin(enable, mt) -- applied for this call and
 *   put back to (-1, 0, 0) / (-1, 0) before it returns; the rest 0.
 * fdesc[4]: x_scale.inv_n, x_scale.eps, r_scale.inv_n, r_scale.eps.
 * in[n][17], host pointers or NULL: 0 a0 fp32 [a0 rows][lda0], 1 a1 [a1 rows][lda1], 2 a0b [a0b rows][lda0], 3 aidx0 [M], 4 aidx1 [M],
 *   5 aidx0b [M], 6 slot_idx [M], 7 row_mask [M], 8 ctx_state [slots][4 x int32], 9 bias [N], 10 resid [M][ldr], 11 p_add [M][ldp],
 *   12 x_scale partials [M][groups], 13 r_scale partials [M][groups], 14 c_state [slots][hidden] (in), 15 reserved, 16 W [K x N] in the
 *   x4 packed fp32 order at the top of csrc/kernels.h.  wt == 1: the binary16 operands are made on the device by launch_cvt_f16, and
 *   for tile_ok == 2 by launch_repack_x32 with binary16 activation rows (a0, a1), as an fp16 engine holds them.
 * out[n][7], host pointers or NULL; every device array behind them is filled with 0xFF bytes before the launch (c_state: the input):
 *   0 out fp32 [R][ldo], R = slots for EPI_SLOT_STORE with slot_idx, else rows_alloc, 1 out16 [R][ldo] binary16, 2 state
 *   [slots][ld_state], 3 state16, 4 c_state [slots][hidden], 5 ssq_out [rows_alloc][N / 32], 6 the partial planes
 *   [8][rows_alloc][N] of an EPI_PARTIAL problem or of a row-epilogue problem that ran as planes + row kernel.
 * plan_out[16]: the capabilities gemm_query found (stream form, GM_KW, GM_PP, 192-column GM_PP), then gemm_plan's route form mode mt
 *   nt zs planes fused error, then 1 when planes + row kernel ran.
 * Returns 0; -1 bad arguments; -2 a HIP call failed; -3 the plan carries an error (nothing launched). */
APRIL_EXPORT int aprilx_run_gemm(const int32_t *desc, const float *fdesc, const void *const *in, void *const *out, int32_t *plan_out);

/* ONE launch of the conv front end (csrc/kernels_misc.hip: conv 1 + 2 with DoubleSwish, then the im2col rows of conv 3) against host
 * arrays, the way the engine launches it (csrc/conv_debug_api.cc; needs a GPU, no model; tests only: tests/conv_ref.py states the
 * mathematics it is compared with).  The weights are transposed on the device first (launch_conv_weight_transpose), as at load.
 * desc[16], int32: 0 segment rows, 1 mel bins, 2..4 the three strides, 5 channels of conv 1, 6 channels of conv 2, 7 M (chunks),
 *   8 ldo (>= 9 x channels of conv 2), 9 rows of the output array (>= M x W3), 10 slots of the ring (0: x is given chunk by chunk),
 *   11 ring_frames (>= segment rows; also with slots == 0, where the engine has a ring all the same); the rest 0.
 * in[8], host pointers: 0 w0 [c0][9], 1 b0 [c0], 2 w1 [c1][c0][9], 3 b1 [c1], 4 x [M][seg][mel] (slots == 0), 5 ring
 *   [slots][ring_frames][mel], 6 slot_idx [M] (each < slots), 7 ring_tail [M] (each < ring_frames).
 * out[3], host pointers: 0 out [rows][ldo], filled with 0xFF bytes before the launch, 1 w0t [9][c0] or NULL, 2 w1t [c0 x 9][c1] or NULL.
 * info[12]: H1 W1 H2 W2 W3 (rows and columns after conv 1 and 2, columns after conv 3), NP = H2 x W2, the second conv's channels per
 *   workgroup of the grouped form, its dynamic shared memory in bytes, the form that runs (1: the many-chunk form, 0: the grouped
 *   form), 1 when the geometry can be launched; the rest 0.
 * Returns 0; -1 bad arguments or a geometry the front end refuses (csrc/conv_front.h: nothing launched); -2 a HIP call failed. */
APRIL_EXPORT int aprilx_run_conv_front(const int32_t *desc, const void *const *in, void *const *out, int32_t *info);
/* The host part of aprilx_run_conv_front alone: fills info[12] from desc[16] and returns 0, or -1 where aprilx_run_conv_front would
 * launch nothing.  No GPU needed; tests only. */
APRIL_EXPORT int aprilx_conv_front_geometry(const int32_t *desc, int32_t *info);

/* Ramp merge, the pure host part: which problems of the NEXT feed's first R macro steps the last R macro steps
 * of a feed of T chunks over L layers can hold.  Writes one record of 3 + 2 R words per window step to out (cap words): own macro step
 * (1-based, L + T - 1 - R + j), own problems in it, guests in it, then the guests as (layer, chunk) pairs, unused words -1.  Returns the
 * number of window steps -- 0 when nothing can be hosted (own + guest problems exceed three somewhere, or L <= 2 R) --, -1 on bad
 * arguments.  No GPU needed; tests only (the engine builds its launch plans from the same function). */
APRIL_EXPORT int aprilx_ramp_window(int L, int T, int R, int32_t *out, int cap);

/* Which weight-stream kernel (csrc/kernels_recur.hip; layer GEMMs at <= 16 rows) takes a layer GEMM of this shape: kind 0 = the
 * one-launch gates GEMM of a chunk step, 1 = its recurrent half (long feeds), 2 = its input half (long feeds), 3 = FFN up,
 * 4 = LSTM projection, 5 = FFN down; K in `kz` slabs, `groups` sum-of-squares partials per row.  Returns 0 when the general GEMM
 * kernels run it, else the form number (3, 1, 4, 5, 2, 6 for the six kinds), -1 on bad arguments.  No GPU needed; tests only. */
APRIL_EXPORT int aprilx_stream_form(int kind, int M, int N, int K, int kz, int groups);

/* ---- input sample rate -------------------------------------------------------------------
 * The reference takes PCM16 at aam_get_sample_rate() only (reference april_api.h:183 aas_feed_pcm16; april-docs/src/python.md:79:
 * other rates give "gibberish or no results").  A session can instead be told the rate of the PCM it will receive; the library
 * converts it to the model's rate on the GPU, inside the ingest, before the filterbank (DESIGN.md section 11 has the contract:
 * Kaiser-windowed sinc, 32 zero crossings per side, cutoff 0.45 x the lower rate; every segment between two flushes is converted
 * as a whole file).  Accepted: 4000 <= rate <= 384000 with L = model rate / gcd <= 4096.                                        */
/* Extends aas_create_session / aas_feed_pcm16: the PCM16 this session receives from now on is at rate_hz.  0 on success; -1 when the
 * rate is refused, or when the session has audio queued or fed since its creation / last completed aas_flush.  The model's rate
 * restores the default path. */
APRIL_EXPORT int aprilx_session_set_input_rate(AprilASRSession session, uint32_t rate_hz);
/* Extends aam_get_sample_rate per session: the rate aas_feed_pcm16 expects for this session. */
APRIL_EXPORT uint32_t aprilx_session_input_rate(AprilASRSession session);
/* The conversion in_rate -> out_rate as the library runs it (no GPU): lmk_out = {L, M, K}; taps (may be NULL) receives the phase
 * table [L][2K] (cap floats).  0, or -1 where aprilx_session_set_input_rate refuses the rate (or cap is too small).
 * in_rate == out_rate: L = M = 1, K = 0. */
APRIL_EXPORT int aprilx_resampler_taps(uint32_t in_rate, uint32_t out_rate, int32_t *lmk_out, float *taps, size_t cap);
/* One whole segment of n samples at in_rate through the device kernel to the model's rate: writes and returns ceil(n L / M)
 * samples (-1 on refusal or cap too small).  Tests only (extends aprilx_run_fbank's parity role to the resampler). */
APRIL_EXPORT int64_t aprilx_resample(AprilASRModel model, uint32_t in_rate, const int16_t *pcm, size_t n, int16_t *out, size_t cap);

/* ---- input format -------------------------------------------------------------------------
 * The reference takes mono PCM16 only (reference april_api.h:183 aas_feed_pcm16).  A session can instead be told the format of the
 * audio it will receive -- G.711 mu-law or A-law, float32, little-endian int16; 1..8 interleaved channels, one of them or their
 * downmix -- and is then fed raw bytes; the library decodes them on the GPU, inside the ingest, in front of the resampler and the
 * filterbank (DESIGN.md section 15 has the contract, bit for bit).  Decoding yields one int16 sample per audio frame, and everything
 * behind it sees exactly what it would have seen had those samples been fed through aas_feed_pcm16.  The format is independent of
 * the input rate (frames per second); the two may be set in either order.                                                        */
enum { APRILX_ENC_S16 = 0, APRILX_ENC_MULAW = 1, APRILX_ENC_ALAW = 2, APRILX_ENC_F32 = 3 };
typedef struct AprilxInputFormat {
    uint32_t size;               /* sizeof(AprilxInputFormat) */
    uint32_t encoding;           /* APRILX_ENC_* */
    uint32_t channels;           /* 1..8, interleaved; a frame is channels x bytes-per-value bytes */
    int32_t channel;             /* 0..channels-1: that channel; -1: the downmix floor((2 S + C) / (2 C)) of the frame's decoded values */
} AprilxInputFormat;
/* The audio this session receives from now on has this format; NULL or {S16, 1, 0} restores the default (mono PCM16: the session runs
 * the path it always ran and no decode work is issued for it).  0 on success; -1 on a wrong size, an encoding > 3, channels outside
 * 1..8, a channel outside -1..channels-1 (nothing changes), or when the session has audio queued or fed since its creation / last
 * completed aas_flush.  The format persists across aas_flush. */
APRIL_EXPORT int aprilx_session_set_input_format(AprilASRSession session, const AprilxInputFormat *format);
/* Reads the session's format into *out: 1 when it has one, 0 when it runs the default (out = {S16, 1, 0}), -1 on bad arguments. */
APRIL_EXPORT int aprilx_session_input_format(AprilASRSession session, AprilxInputFormat *out);
/* aas_feed_pcm16 in bytes: `bytes` bytes of the session's format (a session without one: PCM16).  0, or -1 -- nothing is queued --
 * when that is not a whole number of frames.  On a session WITH a format aas_feed_pcm16, aprilx_feed_many and
 * aprilx_feed_many_pipelined mean "2 x short_count bytes at this pointer"; a partial frame there is logged and that session's feed
 * is dropped. */
APRIL_EXPORT int aprilx_session_feed_bytes(AprilASRSession session, const void *data, size_t bytes);
/* The group feeds in bytes: depth 0 is aprilx_feed_many (blocks; the buffers are lent), depth >= 1 aprilx_feed_many_pipelined (the
 * bytes are copied).  Sessions with and without a format may share a call.  0, or -1 -- nothing is queued for any session -- when
 * one count is not a whole number of its session's frames. */
APRIL_EXPORT int aprilx_feed_many_bytes(size_t n, AprilASRSession *sessions, const void *const *data, const size_t *byte_counts, int depth);
/* The decode contract in plain C++ (no GPU, no model): writes and returns bytes / frame-size samples; -1 on a bad format, a
 * partial frame or cap too small. */
APRIL_EXPORT int64_t aprilx_decode_host(const AprilxInputFormat *format, const void *data, size_t bytes, int16_t *out, size_t cap);
/* The same through the device kernel alone.  Tests only (the role of aprilx_resample). */
APRIL_EXPORT int64_t aprilx_decode(AprilASRModel model, const AprilxInputFormat *format, const void *data, size_t bytes, int16_t *out, size_t cap);
/* Decode launches of one GPU's engine, the frames they decoded (windows overlap: at least the frames fed), and under
 * aprilx_model_profile(model, 1) their time in ms.  0, -1 on bad arguments.  (Not part of AprilxStats: that struct's layout is pinned.) */
APRIL_EXPORT int aprilx_model_decode_stats(AprilASRModel model, int device_index, uint64_t *launches, uint64_t *frames, double *ms);

/* ---- per-token confidence and alternatives ------------------------------------------------
 * AprilToken.logprob (reference april_api.h:118-137) is the raw joiner logit of the token -- the reference does no softmax -- which
 * cannot be compared between tokens, sessions or models.  A session can ask for the log-softmax of every token it delivers, the
 * blank's, and the K best non-blank candidates of the joiner evaluation that produced it; they are computed where the search
 * already reads the logit row, on the GPU, and change no decision (DESIGN.md section 12 has the contract and its error bound).
 * Extends AprilToken through the field the reference reserves: for such a session AprilToken.reserved of every delivered token
 * (partial and final results, provisional tokens included) points to an AprilxTokenInfo that is valid for the duration of the
 * handler call, like the token array itself.  For every other session it stays NULL; AprilToken.logprob is unchanged in both cases. */
typedef struct AprilxTokenInfo {
    uint32_t size;            /* sizeof(AprilxTokenInfo) as the library was built */
    uint32_t n_alt;           /* valid entries below, <= K */
    uint64_t eval_index;      /* ordinal of the session's joiner evaluation that produced the token: the row
                                 aprilx_session_trace_logits would have written for it */
    float lse;                /* log-sum-exp of the evaluation's logits */
    float token_logprob;      /* log-softmax of the token = alt_logit[0] - lse */
    float blank_logprob;      /* log-softmax of the blank */
    float reserved0;
    int32_t alt_id[8];        /* non-blank ids by descending logit; [0] is the token itself */
    float alt_logit[8];       /* their raw logits; log-softmax = alt_logit[i] - lse */
} AprilxTokenInfo;
/* Extends aas_create_session (reference april_api.h:174): 0 = off (default), 1..8 = K.  0 on success; -1 on a bad K or when the session
   has audio queued or fed since its creation / last completed aas_flush (the rule of aprilx_session_set_input_rate). */
APRIL_EXPORT int aprilx_session_set_confidence(AprilASRSession session, int n_alternatives);
/* The session's K (0 = off). */
APRIL_EXPORT int aprilx_session_confidence(AprilASRSession session);
/* Tests only, beside aprilx_run_decide: the side records of n GIVEN logits rows [n][vocab] with K alternatives,
   through the device code the search uses; out = n AprilxTokenInfo (eval_index = row). */
APRIL_EXPORT int aprilx_run_confidence(AprilASRModel model, int n, const float *logits, int k, AprilxTokenInfo *out);

/* ---- phrase boosting ("hot words", contextual biasing) ------------------------------------
 * Vocabulary the model was not tuned for: the caller hands over phrases, each with a boost in logit units, and the search adds the
 * boost to the tokens that continue one of them -- on the GPU, where the arg-max reads the logit row (DESIGN.md section 13 has the
 * contract).  A phrase is a byte string written the way the model's tokens are written (UTF-8, no case folding); one that does not
 * begin with ' ' gets one prepended (phrases start at word boundaries).  No tokeniser is needed: every segmentation of a phrase into
 * the model's tokens is matched.  Negative boosts suppress.  AprilToken.logprob of a session with a set is the value the search
 * compared, bonus included.  Sessions without a set are not affected. */
typedef struct AprilxBias_i *AprilxBias;
/* Builds a set for this model (no GPU needed; works on aprilx_model_load_host models).  NULL and a message in err when refused: no
 * phrases, an empty phrase, one over 256 bytes, a boost that is not finite or beyond +-100, more than 65535 trie states or 4 M token
 * edges, a vocabulary over 8192 tokens.  Phrases that no sequence of the model's tokens can spell are left out and counted
 * (aprilx_bias_info; err then holds a note although the call succeeds). */
APRIL_EXPORT AprilxBias aprilx_bias_create(AprilASRModel model, size_t n, const char *const *phrases, const float *boosts, char *err, size_t err_cap);
/* Strict sets: a CLOSED phrase list (an IVR menu, digit strings, a spelling alphabet, command-and-control).  A session with such a set
 * emits only sequences of its phrases: at every point the search may pick only the tokens that continue a phrase towards its end -- and,
 * at the start and where a phrase has ended, the tokens that begin one --; every other non-blank token takes no part in the arg-max.  The
 * blank stays free, so the session can still say nothing.  Boosts work as in any set (0 is usual here).  A round in which no permitted
 * token has a usable logit resolves to blank.  Confidences of such a session are taken over the blank and the permitted tokens.
 * aprilx_bias_create_ex with flags = 0 is aprilx_bias_create; unknown flag bits are refused; a strict set of which no phrase can be
 * spelled is refused (it would permit nothing). */
#define APRILX_BIAS_STRICT 1u
APRIL_EXPORT AprilxBias aprilx_bias_create_ex(AprilASRModel model, size_t n, const char *const *phrases, const float *boosts, uint32_t flags, char *err,
                                              size_t err_cap);
/* The flags the set was built with (-1: no set). */
APRIL_EXPORT int aprilx_bias_flags(AprilxBias bias);
/* Sessions still using the set keep it alive. */
APRIL_EXPORT void aprilx_bias_free(AprilxBias bias);
/* Trie states and effective token edges of the set; returns the number of phrases left out as unspellable (-1: no set). */
APRIL_EXPORT int aprilx_bias_info(AprilxBias bias, int32_t *states, int64_t *edges);
/* The effective edges of one state, token ids ascending (no GPU): returns their number, -1 on a bad state or when cap is too small
 * (with all three arrays NULL: only the count).  For a strict set these are the permitted tokens of the state. */
APRIL_EXPORT int aprilx_bias_edges(AprilxBias bias, int32_t state, int32_t *tok, int32_t *next, float *bonus, size_t cap);
/* Extends aas_create_session: the session's search uses the set from now on, starting at the root; NULL = off.  0 on success; -1 when
 * the set was built for another token list, the engine already holds 64 different sets in use, or the session has audio queued or fed since its
 * creation / last completed aas_flush (the rule of aprilx_session_set_input_rate). */
APRIL_EXPORT int aprilx_session_set_bias(AprilASRSession session, AprilxBias bias);
/* The trie state as the host's state machine holds it and as the device keeps it for the session's slot: derived independently,
 * must agree; tests only.  Returns 1 when the session has a set, 0 when not. */
APRIL_EXPORT int aprilx_session_bias_state(AprilASRSession session, int32_t *host_state, int32_t *device_state);
/* Tests only: aprilx_run_decide with the set on the rows whose bias_state_io[i] >= 0 (the row's trie state, in and out); -1 = a row
 * without a set.  op 1 returns the states to the root. */
APRIL_EXPORT int aprilx_run_decide_biased(AprilASRModel model, int n, int op, const float *logits, float early_emit, const int32_t *now_ms, int round,
                                          int32_t *state_io, void *records_out, AprilxBias bias, int32_t *bias_state_io);
/* Tests only: aprilx_run_confidence with the set on the rows whose bias_state[i] >= 0 (the row's trie state); -1 = a row without a set. */
APRIL_EXPORT int aprilx_run_confidence_biased(AprilASRModel model, int n, const float *logits, int k, AprilxBias bias, const int32_t *bias_state,
                                              AprilxTokenInfo *out);

/* ---- search options: endpointing and blank penalty -----------------------------------------
 * The reference ends an utterance (FINAL, then SILENCE) 2200 ms after the last token (src/april_session.c:411) and compares the raw
 * blank logit.  A session can have its own values (DESIGN.md section 14 has the contract); they act where the decision is taken, on
 * the GPU, and the host replays the same lines.  With all three at their defaults a session behaves bit for bit as one without options.
 *   endpoint_silence_ms  200 .. 60000, default 2200: the silence after the last token that ends the utterance
 *   max_utterance_ms     0 (off, default) or 1000 .. 600000: a word that begins this long after the utterance's first token finalises
 *                        what came before it (FINAL only: no SILENCE, the context is kept)
 *   blank_penalty        finite, |p| <= 100, default 0: subtracted from the blank logit in the decision's comparisons (positive: fewer
 *                        deletions, more insertions).  AprilToken.logprob, confidences and traced logits keep the raw values. */
typedef struct AprilxSearchOptions {
    uint32_t size;                  /* sizeof(AprilxSearchOptions) as the caller was built; checked */
    uint32_t endpoint_silence_ms;
    uint32_t max_utterance_ms;
    float blank_penalty;
} AprilxSearchOptions;
/* Extends aas_create_session: NULL = back to no options (the defaults).  The options persist across aas_flush.  0 on success; -1, and
 * nothing changes, on a wrong size, a value out of range, or when the session has audio queued or fed since its creation / last
 * completed aas_flush (the rule of aprilx_session_set_input_rate). */
APRIL_EXPORT int aprilx_session_set_search_options(AprilASRSession session, const AprilxSearchOptions *options);
/* The session's options (the defaults when it has none).  Returns 1 when the session has options, 0 when not, -1 on bad arguments.  Only
 * reads: it never waits for queued audio and may be called from the session's own handler. */
APRIL_EXPORT int aprilx_session_search_options(AprilASRSession session, AprilxSearchOptions *out);
/* Tests only, beside aprilx_run_decide_biased: row i decides with opts[i]; opts[i].size == 0 = a row without options.  bias may be NULL
 * (then bias_state_io is ignored).  max_utterance_ms is the host's alone and is ignored here. */
APRIL_EXPORT int aprilx_run_decide_opts(AprilASRModel model, int n, int op, const float *logits, float early_emit, const int32_t *now_ms, int round,
                                        int32_t *state_io, void *records_out, AprilxBias bias, int32_t *bias_state_io, const AprilxSearchOptions *opts);

/* ---- language model: a byte n-gram model of the caller's own text --------------------------
 * "We have a pile of text from our domain; make the recogniser prefer what that text makes likely."  The library estimates a byte-level
 * n-gram model (interpolated Witten-Bell, order 2 .. 8) from plain text and the search adds  w * log P(token text | what was emitted) + b
 * to every non-blank logit -- on the GPU, where the arg-max reads the logit row (DESIGN.md section 20 has the contract).  The text is
 * written the way the model's tokens are written (no case folding); lines are separate utterances; a line holding a byte that no token
 * has is left out and counted.  No tokeniser is needed: the model works on bytes and is independent of the segmentation.
 * AprilToken.logprob of a session with a model is the value the search compared, the LM term included.  Sessions without a model are not
 * affected.  No accuracy is claimed: the default weight is a placeholder until real audio has been run. */
typedef struct AprilxLm_i *AprilxLm;
/* Builds a model for this model's token list (no GPU needed; works on aprilx_model_load_host models).  NULL and a message in err when
 * refused: an order outside 2 .. 8, a token whose text holds the byte 0x0A, a vocabulary over 8192 tokens, a corpus over 64 MiB, more than
 * 4 Mi nodes or 16 Mi arcs, no line left.  Dropped lines are counted (aprilx_lm_info; err then holds a note although the call succeeds). */
APRIL_EXPORT AprilxLm aprilx_lm_create(AprilASRModel model, const void *text, size_t text_len, int order, char *err, size_t err_cap);
/* Sessions still using the model keep it alive. */
APRIL_EXPORT void aprilx_lm_free(AprilxLm lm);
/* Order, nodes, arcs, start node and alphabet size; returns the number of corpus lines left out (-1: no model). */
APRIL_EXPORT int aprilx_lm_info(AprilxLm lm, int32_t *order, int32_t *nodes, int64_t *arcs, int32_t *start, int32_t *alphabet);
/* The automaton (no GPU): node_off [nodes + 1], back / bow [nodes], arc_byte / arc_logp / arc_next [arcs]; any pointer may be NULL.
 * node_cap / arc_cap: the nodes / arcs the arrays hold (node_off one more).  0, or -1 when a capacity is too small. */
APRIL_EXPORT int aprilx_lm_arrays(AprilxLm lm, int32_t *node_off, int32_t *back, float *bow, uint8_t *arc_byte, float *arc_logp, int32_t *arc_next,
                                  float *unk_logp, size_t node_cap, size_t arc_cap);
/* score(state, tok) of the contract as the host walks it: the fp32 sum over the bytes of the token's text and the node reached. */
APRIL_EXPORT int aprilx_lm_score_host(AprilxLm lm, int32_t state, int32_t tok, float *score, int32_t *next);
/* Extends aas_create_session: the session's search uses the model from now on, starting at its start node; NULL = off.  weight: finite,
 * 0 .. 10; token_bonus: finite, |b| <= 100 (added per non-blank token: the counterweight, with the blank penalty, to the model's pull
 * towards the blank).  0 on success; -1 and a logged message when a value is out of range, the model was built for another token list,
 * the engine already holds 8 other models in use, or the session has audio queued or fed since its creation / last completed aas_flush
 * (the rule of aprilx_session_set_input_rate).  A session with a model refuses aprilx_session_snapshot / aprilx_session_restore. */
APRIL_EXPORT int aprilx_session_set_lm(AprilASRSession session, AprilxLm lm, float weight, float token_bonus);
/* The model's node as the host's state machine holds it and as the device keeps it for the session's slot: derived independently, must
 * agree; tests only.  Returns 1 when the session has a model, 0 when not. */
APRIL_EXPORT int aprilx_session_lm_state(AprilASRSession session, int32_t *host_state, int32_t *device_state);
/* Decision launches of the language-model forms issued so far (one captured into a graph counts once), models resident on the device now,
 * model uploads so far: all zero while no session of the engine has had a model. */
APRIL_EXPORT int aprilx_model_lm_stats(AprilASRModel model, int device_index, uint64_t *launches, int32_t *resident, uint64_t *uploads);
/* Tests only: aprilx_run_decide_opts (bias and opts may be NULL) plus the model on the rows whose lm_state_io[i] >= 0 (the row's node, in
 * and out); -1 = a row without a model.  op 1 returns those rows to the start node. */
APRIL_EXPORT int aprilx_run_decide_lm(AprilASRModel model, int n, int op, const float *logits, float early_emit, const int32_t *now_ms, int round,
                                      int32_t *state_io, void *records_out, AprilxBias bias, int32_t *bias_state_io, const AprilxSearchOptions *opts,
                                      AprilxLm lm, int32_t *lm_state_io, float weight, float token_bonus);
/* Tests only: aprilx_run_confidence_biased (bias may be NULL) plus the model on the rows whose lm_state[i] >= 0. */
APRIL_EXPORT int aprilx_run_confidence_lm(AprilASRModel model, int n, const float *logits, int k, AprilxBias bias, const int32_t *bias_state, AprilxLm lm,
                                          const int32_t *lm_state, float weight, float token_bonus, AprilxTokenInfo *out);

/* ---- tracing / statistics ---------------------------------------------------------------*/
/* every joiner evaluation of this session appends `vocab` floats to buf (tests only; chunk steps of a traced session are
   issued eagerly and waited for one by one) */
APRIL_EXPORT void aprilx_session_trace_logits(AprilASRSession session, float *buf, size_t cap_floats, size_t *used_floats);
APRIL_EXPORT uint64_t aprilx_session_chunks(AprilASRSession session);
/* parity tests of the online fbank (reference src/fbank.c:174-349): copies log-mel rows [first, first + n) of everything the
 * session's feature ring has received so far -- real frames and flush padding, in the order the reference's ring sees them --
 * into out[n][mel] and returns the number of rows written so far.  Nothing is copied when the range is not available: rows that have
 * not been written yet (first + n > rows written) return the count as usual -- the caller sees count < first + n -- and rows that
 * have already left the ring (more than ring_frames rows written since `first`) return UINT64_MAX.  n = 0 / out = NULL: only the
 * count.  Waits for the session to be idle.  Chunk j of the session is rows [j * segment_step, j * segment_step + segment_size).  */
APRIL_EXPORT uint64_t aprilx_session_read_frames(AprilASRSession session, uint64_t first, int n, float *out);
/* The token context as the host's result state machine holds it (host_ctx[2]) and the search state the device keeps for the
   session's slot (device_state[4]: context[0], context[1], last active token or -1, time of the last emission in ms).  The two
   contexts are derived independently from the same joiner results (reference context tensor, src/april_session.c:181-196)
   and must agree; tests only. */
APRIL_EXPORT void aprilx_session_context(AprilASRSession session, int32_t *host_ctx, int32_t *device_state);

/* ---- voice activity.  A session that opts in gets SPEECH_START / SPEECH_END events from a detector that runs
 * on the GPU, on the log-mel rows the filterbank has just written: band energy, an exponential average, a running minimum over the
 * last 256..288 frames as the noise floor, two thresholds with onset and hangover counts.  The feature only observes: the session's
 * callbacks, feature rows and chunk count are those of a session without it, and an engine none of whose sessions has opted in
 * launches nothing new.  Times are on the FRAME clock: frame t of the session (real frames since its creation, flush zeros
 * included, never reset) starts at t * frame_shift ms of its audio; AprilToken.time_ms runs on the chunk-stride clock.
 * Events are delivered in frame order, no later than the token callbacks of the chunks that hold their frames, on the thread that
 * delivers those (the caller's for synchronous sessions); aas_flush / a drain returns after every event of the flushed audio.  A
 * flush that completes inside speech closes the segment with a SPEECH_END at frames_seen * frame_shift, and resets the detector. */
typedef struct AprilxVadOptions {
    uint32_t size;                      /* sizeof(AprilxVadOptions) */
    float band_lo_hz, band_hi_hz;       /* 200, 4000: 0 <= lo < hi <= rate / 2, and the band holds at least one mel bin (peak in [lo, hi]) */
    float onset_db, offset_db;          /* 5.0, 3.0: finite, 0 < offset <= onset <= 60; dB of band energy above the noise floor */
    uint32_t onset_ms, hangover_ms;     /* 50, 300: 10..1000 and 10..10000; frames = ms / frame_shift_ms, at least 1 */
    float min_energy;                   /* -12.0: finite; floor of the band-mean log-mel energy (digital silence is -15.94) */
    uint32_t flags;                     /* 0 */
} AprilxVadOptions;
typedef enum AprilxVadEventKind { APRILX_VAD_SPEECH_START = 1, APRILX_VAD_SPEECH_END = 2 } AprilxVadEventKind;
typedef void (*AprilxVadHandler)(void *userdata, int kind, uint64_t time_ms);
typedef struct AprilxVadInfo {
    int32_t b0, b1;                     /* the band: mel bins [b0, b1) */
    int32_t onset_frames, hangover_frames;
    uint64_t frames_seen;               /* real frames of the session since its creation */
    uint64_t speech_frames;             /* frames whose byte had the speech bit, since the detector was last set */
    uint32_t in_speech, segments;       /* the last frame's speech bit; SPEECH_START events since the detector was last set */
} AprilxVadInfo;
/* the plan the kernel works from, and a session's detector state (64 bytes); tests and users of aprilx_vad_host */
typedef struct AprilxVadPlan { int32_t b0, b1; float inv_nb, thr_on, thr_off, min_energy; int32_t onset_frames, hangover_frames; } AprilxVadPlan;
typedef struct AprilxVadState { float s, cur, hist[8]; int32_t cnt, pos, st, run, first, reserved; } AprilxVadState;
/* options = NULL: off.  0, or -1 and nothing changes: a wrong size, a value out of range, non-zero flags, a NULL handler with
 * options, or a session with audio fed since its last completed flush (the rule of aprilx_session_set_search_options).  Setting
 * resets the detector and its counters; frames_seen runs on. */
APRIL_EXPORT int aprilx_session_set_vad(AprilASRSession session, const AprilxVadOptions *options, AprilxVadHandler handler, void *userdata);
/* 1 and the options / info when the detector is on, 0 (info: frames_seen only) when it is off, -1 on bad arguments; either pointer
 * may be NULL.  Waits for the session to be idle. */
APRIL_EXPORT int aprilx_session_vad(AprilASRSession session, AprilxVadOptions *options_out, AprilxVadInfo *out);
/* The plan from a mel table mel[nbins][nfft_bins] (aprilx_model_fbank_tables: nfft_bins = fft_size / 2): 0, or -1 as above.  No GPU. */
APRIL_EXPORT int aprilx_vad_plan_tables(const float *mel, int nbins, int nfft_bins, int sample_rate, int frame_shift_ms,
                                        const AprilxVadOptions *options, AprilxVadPlan *plan_out);
/* The contract on the host: n rows of nbins floats through steps 1-9 from *state_inout (reset state: cur and hist +inf, first 1,
 * the rest 0), one byte per row (bit 0 speech, bit 1 raw), energy_out (may be NULL) step 1's band mean of every row.  No GPU. */
APRIL_EXPORT int aprilx_vad_host(const AprilxVadPlan *plan, int n, int nbins, const float *rows, AprilxVadState *state_inout, uint8_t *bytes_out,
                                 float *energy_out);
/* Events from the bytes of frames [t0, t0 + n), last_bit the speech bit of frame t0 - 1: kinds_out / times_out (cap entries each)
 * receive them in order; returns their number (may exceed cap: nothing is written past it), *last_bit the new one.  No GPU. */
APRIL_EXPORT int aprilx_vad_events_host(const AprilxVadPlan *plan, int frame_shift_ms, uint64_t t0, const uint8_t *bytes, size_t n, int32_t *last_bit,
                                        int32_t *kinds_out, uint64_t *times_out, int cap);
/* Tests only: vad_kernel on n_runs runs in ONE launch over a scratch ring of R = max(n[]) rows per run.  Run r has its own options
 * (as a plan derived from the model's tables), n[r] rows -- consecutive in rows[sum n][mel] -- placed at ring rows
 * (first_row[r] + i) % R (0 <= first_row[r] < R: a run that wraps), and its state states_inout[r].  bytes_out / energy_out[sum n].
 * 0, or -1 on bad arguments. */
APRIL_EXPORT int aprilx_run_vad(AprilASRModel model, int n_runs, const AprilxVadOptions *options, const int32_t *n, const int32_t *first_row,
                                const float *rows, AprilxVadState *states_inout, uint8_t *bytes_out, float *energy_out);
/* VAD launches and the frames they covered on one GPU's engine, and (while profiling) the kernel's accumulated ms.  0, or -1. */
APRIL_EXPORT int aprilx_model_vad_stats(AprilASRModel model, int device_index, uint64_t *launches, uint64_t *frames, double *ms);

/* ---- DTMF.  A session that opts in gets key-down / key-up events for in-band DTMF digits from a detector that
 * runs on the GPU, on the model-rate samples the filterbank reads (after decode and resampling): per frame the correlation of its first
 * Wd samples with the eight DTMF frequencies, level, twist, peak and energy-share checks -> one code per frame; the host turns
 * consecutive codes into events.  The feature only observes, as voice activity does, and an engine none of whose sessions has opted in
 * launches and copies nothing new.  Times are on the FRAME clock of the voice-activity events; delivery follows their rules.  A flush
 * that completes inside a held digit closes it with an UP at frames_seen * frame_shift, and resets the machine.  The digits are
 * "123A456B789C*0#D"[code - 1].  Second-harmonic talk-off rejection is not part of the contract. */
typedef struct AprilxDtmfOptions {
    uint32_t size;                      /* sizeof(AprilxDtmfOptions) */
    float min_level_dbfs;               /* -40: -70..0; level floor per tone */
    float twist_hi_db, twist_lo_db;     /* 4, 8: 0..20; column group over row group, row group over column group */
    float rel_peak_db;                  /* 8: 3..30; the peak over the other rows / columns */
    float min_share;                    /* 0.6: 0 < s <= 1; share of the frame's energy in the two tones */
    uint32_t min_tone_ms, min_pause_ms; /* 20, 20: 10..1000; frames = ms / frame_shift_ms, at least 1 */
    uint32_t flags;                     /* 0 */
} AprilxDtmfOptions;
enum { APRILX_DTMF_DOWN = 1, APRILX_DTMF_UP = 2 };
typedef void (*AprilxDtmfHandler)(void *userdata, int kind, char digit, uint64_t time_ms);
typedef struct AprilxDtmfInfo {
    int32_t Wd, on_frames, off_frames;
    uint32_t held;                      /* the digit held after the last frame read (a character), or 0 */
    uint64_t frames_seen;               /* real frames of the session since its creation */
    uint64_t tone_frames;               /* frames with a non-zero code, since the detector was last set */
    uint64_t digits;                    /* DOWN events since the detector was last set */
} AprilxDtmfInfo;
/* the plan the kernel and the event machine work from (40 bytes); tests and users of aprilx_dtmf_host */
typedef struct AprilxDtmfPlan {
    int32_t Wd; float half_w, min_power, twist_hi, twist_lo, rel_peak, min_share; int32_t on_frames, off_frames, reserved;
} AprilxDtmfPlan;
/* the event machine's state between calls of aprilx_dtmf_events_host: all zero at the start and after a flush */
typedef struct AprilxDtmfMachine { int32_t held, cand, run; } AprilxDtmfMachine;
/* options = NULL: off.  0, or -1 and nothing changes: a wrong size, a value out of range, non-zero flags, a NULL handler with options,
 * a model the detector refuses (a window Wd / rate below 12 ms, a rate below 4000 Hz, Wd above 4096), or a session with audio fed
 * since its last completed flush (the rule of aprilx_session_set_vad).  Setting resets the machine and its counters. */
APRIL_EXPORT int aprilx_session_set_dtmf(AprilASRSession session, const AprilxDtmfOptions *options, AprilxDtmfHandler handler, void *userdata);
/* 1 and the options / info when the detector is on, 0 (info: frames_seen only) when it is off, -1 on bad arguments; either pointer
 * may be NULL.  Waits for the session to be idle. */
APRIL_EXPORT int aprilx_session_dtmf(AprilASRSession session, AprilxDtmfOptions *options_out, AprilxDtmfInfo *out);
/* The plan of a model with this rate, fft size (aprilx_model_fbank_tables: 2 nfft_bins) and frame shift: 0, or -1 as above.  No GPU. */
APRIL_EXPORT int aprilx_dtmf_plan(int sample_rate, int fft_size, int frame_shift_ms, const AprilxDtmfOptions *options, AprilxDtmfPlan *plan_out);
/* The tables [16][Wd] (rows 0..7 cos, 8..15 sin of the eight frequencies) into out[cap]: 16 Wd, or -1 (cap too small, bad Wd).  No GPU. */
APRIL_EXPORT int aprilx_dtmf_tables(int sample_rate, int Wd, float *out, size_t cap);
/* The contract on the host: frame i at frames + i * ld (ld >= Wd samples) through steps 1-5; codes_out[n], powers_out [n][9]
 * (P[0..8) and E) or NULL.  No GPU. */
APRIL_EXPORT int aprilx_dtmf_host(const AprilxDtmfPlan *plan, const float *tables, int n, const int16_t *frames, size_t ld, uint8_t *codes_out,
                                  float *powers_out);
/* steps 3-4 on one row of P[0..8), E: the code, or -1 on bad arguments.  No GPU. */
APRIL_EXPORT int aprilx_dtmf_decide_host(const AprilxDtmfPlan *plan, const float *powers9);
/* Events from the codes of frames [t0, t0 + n) from *machine: kinds_out / digits_out / times_out (cap entries each) receive them in
 * order; flush != 0: a flush then completes at frame t0 + n.  Returns their number (may exceed cap: nothing is written past it).  No GPU. */
APRIL_EXPORT int aprilx_dtmf_events_host(const AprilxDtmfPlan *plan, int frame_shift_ms, uint64_t t0, const uint8_t *codes, size_t n, int flush,
                                         AprilxDtmfMachine *machine, int32_t *kinds_out, char *digits_out, uint64_t *times_out, int cap);
/* Tests only: dtmf_kernel on n_runs runs in ONE launch.  Run r has its own options and n[r] frames, consecutive in
 * frames[sum n][fft_size] as for aprilx_run_fbank; codes_out[sum n], powers_out [sum n][9] or NULL.  0, or -1 on bad arguments. */
APRIL_EXPORT int aprilx_run_dtmf(AprilASRModel model, const AprilxDtmfOptions *options, int n_runs, const int32_t *n, const int16_t *frames,
                                 uint8_t *codes_out, float *powers_out);
/* Tests only: the kernel's decision alone on n given rows of P[0..8), E.  0, or -1. */
APRIL_EXPORT int aprilx_run_dtmf_decide(AprilASRModel model, const AprilxDtmfOptions *options, int n, const float *powers9, uint8_t *codes_out);
/* DTMF launches and the frames they covered on one GPU's engine, and (while profiling) the kernel's accumulated ms.  0, or -1. */
APRIL_EXPORT int aprilx_model_dtmf_stats(AprilASRModel model, int device_index, uint64_t *launches, uint64_t *frames, double *ms);

/* ---- Tones.  A session that opts in gets ON / OFF events for sustained tones -- the beep of an answering machine,
 * fax CNG and CED, dial tone, busy and reorder, the 425 Hz tones of European networks, the segments of a special-information tone --
 * from a detector that runs on the GPU, on the model-rate samples the filterbank reads: per frame the correlation of its first
 * W = 64 floor(fft_size / 64) samples with every DFT bin of length W from 300 to 2300 Hz, the strongest bin and the strongest one at
 * least three bins away, level, second-component and energy-share checks, and an interpolated frequency per component -> one record of
 * two uint16 per frame ((hz, 0) a single tone, (lo, hi) a pair, (0, 0) none); the host turns consecutive records into events.  The
 * frequencies are not fixed in advance: an event carries what was measured, and aprilx_tone_name() names the well-known ones.
 * CADENCE IS THE CALLER'S: busy and reorder are the same pair at different rhythms, ringing is a tone that comes and goes; read them from
 * the ON / OFF times.  Two components closer than three bins (93.75 Hz at 16 kHz / 512) are ONE tone: North American ringback
 * (440 + 480 Hz), and dial tone on a model whose frames are not rounded up to a power of two.  Whistling and sung notes are tones.  A
 * DTMF digit is a pair inside the grid and is reported here too, beside the DTMF detector's own event; neither suppresses the other.
 * The feature only observes, as voice activity and DTMF do, and an engine none of whose sessions has opted in launches, copies and
 * allocates nothing new.  Times are on the FRAME clock of the voice-activity events; delivery follows their rules.  A flush that
 * completes inside a held tone closes it with an OFF at frames_seen * frame_shift, and resets the machine. */
typedef struct AprilxToneOptions {
    uint32_t size;                      /* sizeof(AprilxToneOptions) */
    float min_level_dbfs;               /* -40: -70..0; level floor of the strongest component */
    float second_db;                    /* 10: 3..30; how far the second component may lie below the first and still make a pair */
    float min_share;                    /* 0.7: 0 < s <= 1; share of the frame's energy in the component(s) */
    uint32_t tol_hz;                    /* 20: 1..200; two records are the same tone when each frequency differs by at most this */
    uint32_t min_tone_ms, min_pause_ms; /* 60, 30: 10..5000; frames = ms / frame_shift_ms, at least 1 */
    uint32_t flags;                     /* 0 */
} AprilxToneOptions;
enum { APRILX_TONE_ON = 1, APRILX_TONE_OFF = 2 };
/* a single tone: f2_hz == 0; a pair: f1_hz < f2_hz (OFF carries the frequencies its ON carried) */
typedef void (*AprilxToneHandler)(void *userdata, int kind, uint32_t f1_hz, uint32_t f2_hz, uint64_t time_ms);
typedef struct AprilxToneInfo {
    int32_t W, k_lo, F, on_frames, off_frames;
    uint32_t held_f1, held_f2;          /* the tone held after the last frame read, or 0, 0 */
    uint32_t reserved;
    uint64_t frames_seen;               /* real frames of the session since its creation */
    uint64_t tonal_frames;              /* frames with a tonal record, since the detector was last set */
    uint64_t tones;                     /* ON events since the detector was last set */
} AprilxToneInfo;
/* the plan the kernel and the event machine work from (48 bytes); tests and users of aprilx_tone_host */
typedef struct AprilxTonePlan {
    int32_t W, k_lo, F; float half_w, min_power, second_ratio, min_share, bin_hz; int32_t tol_hz, on_frames, off_frames, reserved;
} AprilxTonePlan;
/* the event machine's state between calls of aprilx_tone_events_host: all zero at the start and after a flush */
typedef struct AprilxToneMachine { int32_t held, h1, h2, c1, c2, run; } AprilxToneMachine;
/* options = NULL: off.  0, or -1 and nothing changes: a wrong size, a value out of range, non-zero flags, a NULL handler with options,
 * a model the detector refuses (W / rate below 20 ms, a rate below 6000 Hz, W above 4096, a grid of fewer than 8 or more than 128
 * bins), or a session with audio fed since its last completed flush (the rule of aprilx_session_set_vad).  Setting resets the machine
 * and its counters. */
APRIL_EXPORT int aprilx_session_set_tones(AprilASRSession session, const AprilxToneOptions *options, AprilxToneHandler handler, void *userdata);
/* 1 and the options / info when the detector is on, 0 (info: frames_seen only) when it is off, -1 on bad arguments; either pointer
 * may be NULL.  Waits for the session to be idle. */
APRIL_EXPORT int aprilx_session_tones(AprilASRSession session, AprilxToneOptions *options_out, AprilxToneInfo *out);
/* The plan of a model with this rate, fft size and frame shift: 0, or -1 as above.  No GPU. */
APRIL_EXPORT int aprilx_tone_plan(int sample_rate, int fft_size, int frame_shift_ms, const AprilxToneOptions *options, AprilxTonePlan *plan_out);
/* The tables [2F][W] (row k cos, row F + k sin of bin k_lo + k) into out[cap]: 2 F W, or -1 (cap too small, a refused model).  No GPU. */
APRIL_EXPORT int aprilx_tone_tables(int sample_rate, int fft_size, float *out, size_t cap);
/* The contract on the host: frame i at frames + i * ld (ld >= W samples) through steps 1-7; records_out [n][2] uint16, powers_out
 * [n][F + 1] (P[0..F) and E) or NULL.  No GPU. */
APRIL_EXPORT int aprilx_tone_host(const AprilxTonePlan *plan, const float *tables, int n, const int16_t *frames, size_t ld, uint16_t *records_out,
                                  float *powers_out);
/* steps 3-7 on one row of P[0..F), E (F + 1 values): the record as lo | hi << 16, or -1 on bad arguments.  No GPU. */
APRIL_EXPORT int64_t aprilx_tone_decide_host(const AprilxTonePlan *plan, const float *powers);
/* Events from the records ([n][2] uint16) of frames [t0, t0 + n) from *machine: kinds_out / f1_out / f2_out / times_out (cap entries
 * each) receive them in order; flush != 0: a flush then completes at frame t0 + n.  Returns their number (may exceed cap: nothing is
 * written past it).  No GPU. */
APRIL_EXPORT int aprilx_tone_events_host(const AprilxTonePlan *plan, int frame_shift_ms, uint64_t t0, const uint16_t *records, size_t n, int flush,
                                         AprilxToneMachine *machine, int32_t *kinds_out, uint32_t *f1_out, uint32_t *f2_out, uint64_t *times_out, int cap);
/* "dial" 350 + 440, "busy" 480 + 620, "cp425" 425, "cng" 1100, "ced" 2100, "sit1" 950, "sit2" 1400, "sit3" 1800 Hz: the static name
 * of the first entry all of whose frequencies lie within tol_hz of the given ones, or NULL. */
APRIL_EXPORT const char *aprilx_tone_name(uint32_t f1_hz, uint32_t f2_hz, uint32_t tol_hz);
/* Tests only: tone_kernel on n_runs runs in ONE launch.  Run r has its own options and n[r] frames, consecutive in
 * frames[sum n][fft_size] as for aprilx_run_fbank; records_out [sum n][2], powers_out [sum n][F + 1] or NULL.  0, or -1 on bad arguments. */
APRIL_EXPORT int aprilx_run_tones(AprilASRModel model, const AprilxToneOptions *options, int n_runs, const int32_t *n, const int16_t *frames,
                                  uint16_t *records_out, float *powers_out);
/* Tests only: the kernel's decision alone on n given rows of P[0..F), E; records_out [n][2].  0, or -1. */
APRIL_EXPORT int aprilx_run_tone_decide(AprilASRModel model, const AprilxToneOptions *options, int n, const float *powers, uint16_t *records_out);
/* Tone launches and the frames they covered on one GPU's engine, and (while profiling) the kernel's accumulated ms.  0, or -1. */
APRIL_EXPORT int aprilx_model_tone_stats(AprilASRModel model, int device_index, uint64_t *launches, uint64_t *frames, double *ms);

/* ---- Line quality.  Why is this stream's transcript bad?  Usually the signal: a caller 30 dB too quiet, a gateway
 * that clips, a one-way leg (digital silence, or a stuck value a concealer filled in), a large DC offset, a noise floor a few dB under the
 * speech.  A session that opts in gets periodic REPORTs and CLIPPING / DROPOUT ON / OFF events from an observer that runs on the GPU, on
 * the model-rate int16 samples the filterbank reads -- which the host never sees for a stream that feeds mu-law at 8 kHz.  Real frame t
 * owns the hop x[0 .. H), the first H = frame_shift_ms * rate / 1000 samples of its frame: hops do not overlap, sums over frames are sums
 * over the audio.  Per frame the device writes one record of eight little-endian uint32, integers only: sumsq (64 bits, low word
 * first), sum (int32), (uint16)min | (uint16)max << 16, clip_count | clip_run << 16 (samples with x >= L or x <= -L, and the longest
 * run of consecutive such samples INSIDE the hop; L the session's clip level), 1 if min == max (a dead frame) else 0, and two zero
 * words.  The host turns consecutive records into events:
 *   CLIPPING  a frame is clipped when clip_run >= clip_run_min.  ON at the first clipped frame (time t * shift); OFF once
 *             clip_hold_ms / shift consecutive unclipped frames have passed, at the time of the first of them.
 *   DROPOUT   ON once dropout_ms / shift consecutive dead frames have passed, at the time of the first of them; OFF at the first live frame.
 *   REPORT    one per report_ms / shift frames, from frame 0 of the options' life, at the time of its first frame, with the sums below.
 * A frame's events come in that order.  A flush that completes closes whatever is on with an OFF at frames_seen * frame_shift, then the
 * open interval with a short REPORT, and resets the machine.  Levels in dB are derived from the integers by the caller
 * (rms_dbfs = 10 log10(sumsq / (frames * hop) / 32768^2)).  The figures describe the MODEL-RATE stream: clipping in a source at another
 * rate is smeared by the resampler; a G.711 line never reaches 32767 -- set clip_level 32124 for mu-law, 32256 for A-law.  Runs are not
 * followed across a hop boundary.  loud_sumsq / quiet_sumsq is a loudest-to-quietest-frame ratio inside one interval, not a speech SNR.
 * The feature only observes, as the detectors do, and an engine none of whose sessions has opted in launches, copies and allocates
 * nothing new.  Times are on the FRAME clock of the voice-activity events; delivery follows their rules. */
typedef struct AprilxQualityOptions {
    uint32_t size;                      /* sizeof(AprilxQualityOptions) */
    uint32_t flags;                     /* 0 */
    uint32_t clip_level;                /* 32767: 1024..32767; a sample is clipped when x >= clip_level or x <= -clip_level */
    uint32_t clip_run_min;              /* 3: 1..64; a frame is clipped when its longest run has at least this many samples */
    uint32_t clip_hold_ms;              /* 1000: 100..60000 */
    uint32_t dropout_ms;                /* 200: 20..60000 */
    uint32_t report_ms;                 /* 1000: 0 (no reports) or 100..60000 */
} AprilxQualityOptions;
enum { APRILX_QUALITY_REPORT = 1, APRILX_QUALITY_CLIPPING_ON = 2, APRILX_QUALITY_CLIPPING_OFF = 3, APRILX_QUALITY_DROPOUT_ON = 4, APRILX_QUALITY_DROPOUT_OFF = 5 };
/* one event (80 bytes); the fields behind time_ms are a REPORT's and zero otherwise */
typedef struct AprilxQualityEvent {
    int32_t kind;
    uint32_t frames;                    /* frames of the interval */
    uint64_t time_ms;
    int64_t sum;                        /* of all samples of the interval */
    uint64_t sumsq;
    int32_t min, max;
    uint64_t clip_samples;
    uint32_t clipped_frames, dead_frames;
    uint64_t quiet_sumsq, loud_sumsq;   /* the smallest frame sumsq among the interval's live frames (0: none), the largest of all its frames */
    uint32_t hop, reserved;             /* samples per frame (every event carries it) */
} AprilxQualityEvent;
/* the event is valid during the call only */
typedef void (*AprilxQualityHandler)(void *userdata, const AprilxQualityEvent *event);
typedef struct AprilxQualityInfo {
    int32_t hop, hold_frames, dropout_frames, report_frames;
    uint32_t clipping, dropout;         /* what is on after the last frame read */
    uint64_t frames_seen;               /* real frames of the session since its creation */
    uint64_t frames, clipped_frames, dead_frames, clip_samples, reports;      /* since the observer was last set */
} AprilxQualityInfo;
/* what kernel and machine work from (24 bytes); tests and users of aprilx_quality_events_host */
typedef struct AprilxQualityPlan { int32_t hop, clip_level, clip_run_min, hold_frames, dropout_frames, report_frames; } AprilxQualityPlan;
/* the machine's state between calls of aprilx_quality_events_host (88 bytes): all zero at the start and after a flush */
typedef struct AprilxQualityMachine {
    int32_t clipping, dropout, quiet_run, dead_run; uint32_t frames; int32_t have_live; uint64_t first_frame; int64_t sum; uint64_t sumsq;
    int32_t min, max; uint64_t clip_samples; uint32_t clipped_frames, dead_frames; uint64_t quiet_sumsq, loud_sumsq;
} AprilxQualityMachine;
/* options = NULL: off.  0, or -1 and nothing changes: a wrong size, a value out of range, non-zero flags, a NULL handler with options, a
 * model whose hop is longer than its frame or than 32767 samples, or a session with audio fed since its last completed flush (the rule
 * of aprilx_session_set_input_rate).  Setting resets the machine and its counters.  A session with the observer on is refused by
 * aprilx_session_snapshot and as a target of aprilx_session_restore: the snapshot format does not carry the machine. */
APRIL_EXPORT int aprilx_session_set_quality(AprilASRSession session, const AprilxQualityOptions *options, AprilxQualityHandler handler, void *userdata);
/* 1 and the options / info when the observer is on, 0 (info: frames_seen only) when it is off, -1 on bad arguments; either pointer may
 * be NULL.  Waits for the session to be idle. */
APRIL_EXPORT int aprilx_session_quality(AprilASRSession session, AprilxQualityOptions *options_out, AprilxQualityInfo *out);
/* The plan of a model with this rate, frame length (samples the filterbank reads per frame) and frame shift: 0, or -1 as above.  No GPU. */
APRIL_EXPORT int aprilx_quality_plan(int sample_rate, int frame_samples, int frame_shift_ms, const AprilxQualityOptions *options, AprilxQualityPlan *plan_out);
/* The records on the host: hop i is the first `hop` samples at frames + i * ld (ld >= hop); records_out [n][8] uint32.  hop 1..32767,
 * clip_level 1024..32767.  0, or -1.  No GPU. */
APRIL_EXPORT int aprilx_quality_host(int hop, int clip_level, int n, const int16_t *frames, size_t ld, uint32_t *records_out);
/* Events from the records ([n][8] uint32) of frames [t0, t0 + n) from *machine: events_out (cap entries) receives them in order;
 * flush != 0: a flush then completes at frame t0 + n.  Returns their number (may exceed cap: nothing is written past it), or -1.  No GPU. */
APRIL_EXPORT int aprilx_quality_events_host(const AprilxQualityPlan *plan, int frame_shift_ms, uint64_t t0, const uint32_t *records, size_t n, int flush,
                                            AprilxQualityMachine *machine, AprilxQualityEvent *events_out, int cap);
/* Tests only: quality_kernel on n_runs runs in ONE launch.  Run r has its own clip level and n[r] frames, consecutive in
 * frames[sum n][fft_size] as for aprilx_run_fbank; records_out [sum n][8].  0, or -1 on bad arguments. */
APRIL_EXPORT int aprilx_run_quality(AprilASRModel model, const int32_t *clip_levels, int n_runs, const int32_t *n, const int16_t *frames, uint32_t *records_out);
/* Quality launches and the frames they covered on one GPU's engine, and (while profiling) the kernel's accumulated ms: all zero in an
 * engine without an opted-in session.  0, or -1. */
APRIL_EXPORT int aprilx_model_quality_stats(AprilASRModel model, int device_index, uint64_t *launches, uint64_t *frames, double *ms);

/* ---- session snapshot and restore.  A stream is otherwise pinned to the slot, engine and process that created
 * it.  A snapshot is a self-contained blob of everything dynamic a session holds at an IDLE point -- the slot's recurrent state, the
 * encoder / decoder outputs, the search and trie state, the detectors' state, the feature-ring rows not yet consumed, the host's result
 * state machine, the unconsumed audio tail and the counters -- plus the configuration and the model's identity.  Restored into a fresh
 * session of the same model and precision that was configured the same way, the stream continues bit for bit: fed the same remaining
 * audio in the same feed sizes it delivers the same callbacks, events, feature rows and counters as the source would have.  The blob
 * is little-endian bytes ("APXSNAP1", a version, the total size, block offsets, FNV-1a 64 over everything before the trailing hash);
 * moving it is the caller's.  NOT carried: handlers and userdata, the bias set itself (only its identity), logit tracing, the latency
 * ring, aas_realtime_get_speedup's average.  AprilConfig.speaker stays ignored.
 * The device part of n sessions moves in ONE gather (or scatter) kernel launch and one staging copy per engine per call, on the
 * engine's stepping thread between flights. */
typedef struct AprilxSnapshotInfo {
    uint32_t size;                  /* sizeof(AprilxSnapshotInfo) */
    uint32_t version;               /* blob format version: 1 */
    uint64_t blob_size;
    uint64_t params_hash;           /* FNV-1a 64 of the model's PARAMS fields (the 13 int32 of the reference's params block, in its order) */
    uint64_t token_hash;            /* of the token list (the hash bias sets are checked with) */
    uint64_t bias_hash;             /* FNV-1a 64 of the set's state_off, edge_tok, edge_next and edge_bonus arrays; 0 without a set */
    int64_t bias_edges;
    uint64_t chunks, frames_seen, now_ms, rows_written;   /* where the stream stands */
    int32_t n_layers, d_model, hidden, ffn, joiner, vocab, mel, segment_size, segment_step, sample_rate, frame_shift_ms, blank_id;
    uint32_t precision;             /* 0 fp32, 1 fp16 operands */
    uint32_t f16_tile;              /* the engine keeps a binary16 copy of h, which the blob carries */
    uint32_t input_rate;            /* Hz: what aprilx_session_input_rate returns */
    uint32_t confidence_k;
    uint32_t has_format, has_search_options, has_vad, has_dtmf, has_tones, has_bias;      /* 0 / 1: the structs below are meaningful */
    uint32_t bias_flags; int32_t bias_states;
    uint32_t ring_rows;             /* feature-ring rows in the blob */
    uint32_t reserved;
    AprilxInputFormat format;
    AprilxSearchOptions search;
    AprilxVadOptions vad;
    AprilxDtmfOptions dtmf;
    AprilxToneOptions tones;
    char name[64], description[128];   /* aam_get_name / aam_get_description, truncated, NUL padded */
} AprilxSnapshotInfo;
/* Waits until the session is idle -- everything queued has been processed and its events delivered, as aprilx_session_drain does --,
 * then writes the blob and leaves the session as it is (it may go on, or be freed).  dst == NULL: returns the bytes needed.  Else the
 * bytes written, or -1: cap too small, a flush under way, or called from a handler of the session. */
APRIL_EXPORT int64_t aprilx_session_snapshot(AprilASRSession session, void *dst, size_t cap);
/* Loads a blob into a FRESH session (never fed since its creation) of the same model and precision whose input rate, format, K, search
 * options, detectors and bias set were set as the source's were.  0, or -1 with a message in err (may be NULL): a corrupt blob, another
 * model or precision, a configuration that differs, a session that was fed.  A refused session is untouched and usable. */
APRIL_EXPORT int aprilx_session_restore(AprilASRSession session, const void *blob, size_t size, char *err, size_t err_cap);
/* The configuration, identity and progress stored in a blob, so that a receiver can configure its session from the blob alone (the bias
 * set is the caller's to rebuild).  Needs no GPU and no model.  0, or -1 on a blob that does not parse (never reads past size). */
APRIL_EXPORT int aprilx_snapshot_info(const void *blob, size_t size, AprilxSnapshotInfo *out);
/* Both for n sessions at once, grouped by engine inside: one gather / scatter launch per engine.  snapshot_many: caps[i] bytes at dsts[i]
 * (dsts == NULL: only sizes_out), sizes_out[i] = bytes written / needed, or -1.  restore_many: status_out[i] = 0 or -1.  Both return the
 * number of sessions that failed. */
APRIL_EXPORT int aprilx_snapshot_many(size_t n, AprilASRSession *sessions, void *const *dsts, const size_t *caps, int64_t *sizes_out);
APRIL_EXPORT int aprilx_restore_many(size_t n, AprilASRSession *sessions, const void *const *blobs, const size_t *sizes, int *status_out);
/* Gather and scatter launches of one GPU's engine so far, and (while profiling) their accumulated kernel ms.  0, or -1. */
APRIL_EXPORT int aprilx_model_snapshot_stats(AprilASRModel model, int device_index, uint64_t *gathers, uint64_t *scatters, double *gather_ms, double *scatter_ms);

typedef struct AprilxStats {
    uint64_t ticks, steps, chunks, rounds, frames, max_batch_seen;
    /* per kernel class: accumulated ms and launch counts while profiling is enabled
       0 gates GEMM+LSTM cell, 1 other encoder GEMMs, 2 row epilogues, 3 conv front end, 4 fbank, 5 decoder+joiner */
    double kernel_ms[6];
    uint64_t kernel_launches[6];
    /* host wall time of the GPU's stepping thread by phase (ms): 0 collect work, 1 frame bookkeeping, 2 fbank call,
       3 chunk-step enqueue, 4 end of flight (the one wait for the GPU), 5 replay of the device's per-round records through
       the result state machine, 6 decoder refresh enqueue, 7 completion */
    double host_ms[8];
    uint64_t flights;            /* host waits for the GPU (one per flight = per batch of queued chunk steps) */
    uint64_t replay_mismatch;    /* rounds where the host state machine and the device decision disagreed (must stay 0) */
    uint64_t kernels_per_step;   /* launches of the last eagerly issued chunk chain (profiling / APRIL_NO_GRAPHS runs) */
    uint64_t lm_steps, lm_chunks;/* layer-major steps (long feeds) and the session-chunks they covered (included in steps / chunks) */
    uint64_t wave_steps, wave_chunks;/* feeds whose 2..7 chunk steps ran as one wavefront over the layers, and the session-chunks they covered (included in steps / chunks) */
    /* the gates clock (aprilx_model_profile(model, 2) ... (model, 0)): every gates launch of the feed wavefronts timed ITSELF under graph
       replay (first workgroup's start to last workgroup's end, s_memrealtime) -- accumulated ms, launches and rows (sessions x layers
       sharing the launch) of the last clocked interval */
    double gates_clock_ms; uint64_t gates_clock_launches, gates_clock_rows;
    double gates_clock_ms_by_n[4]; uint64_t gates_clock_launches_by_n[4];   /* the same, split by the problems sharing the launch (1, 2, 3, >= 4) */
    double resample_ms; uint64_t resample_launches;   /* profiling: the resample launches of sessions with an input rate of their own (before the fbank) */
    uint64_t confidence_records; /* side records (aprilx_session_set_confidence) copied to the host so far; 0 while no session has opted in */
} AprilxStats;
APRIL_EXPORT void aprilx_model_stats(AprilASRModel model, int device_index, AprilxStats *out);
/* Ramp merge counters of one GPU's engine: *ramp_eligible = split feeds launched with nothing enqueued on the layer stream since the
 * previous feed's layer graph (only those can be hosted), *ramp_hosted = feeds whose first two macro steps ran inside the previous
 * feed's last two (counted on the device by the kernel that decides it; exact once the streams are idle).  Returns 0, -1 on bad
 * arguments.  (Not part of AprilxStats: that struct's layout is pinned.) */
APRIL_EXPORT int aprilx_model_ramp_stats(AprilASRModel model, int device_index, uint64_t *ramp_hosted, uint64_t *ramp_eligible);
/* The same two counters and those of the deferred enqueue (APRIL_RAMP_MERGE=1), out[0..4]: hosted, eligible (there: feeds
 * whose layer graph waited for the latch's report), headless layer graphs launched (= hosted once the streams are idle), deferrals settled by
 * the stepping thread's wait for a flight (wait_flight / flight_done), deferrals settled by any other engine entry (the launch itself when the
 * report was already there, a slot reset, an upload, the next flight).  Returns 0, -1 on bad arguments. */
APRIL_EXPORT int aprilx_model_ramp_stats2(AprilASRModel model, int device_index, uint64_t out[5]);
/* Hand-over -> delivery latency of the last (up to 8192) completed ticks of one GPU's stepping thread, in ms, oldest first: from the
 * feed call (aas_feed_pcm16 / aprilx_feed_many / aprilx_feed_many_pipelined / flush) that queued the oldest work a flight served to
 * the moment that flight's results were delivered (asynchronous and pipelined sessions: their handlers have run; synchronous callers:
 * released).  With the pipelined group feed the duration of the feed CALL is only the hand-over; this is the latency a client sees
 * (reference: the time aas_feed_pcm16 blocks, src/april_session.c:479-538).  out_ms = NULL: returns the number available; reset != 0
 * empties the ring afterwards.                                                                                                    */
APRIL_EXPORT int aprilx_model_feed_latency(AprilASRModel model, int device_index, double *out_ms, int cap, int reset);
/* enable 1: launches go out one by one with hipEvents around them on the engine's stream (gates launches: their own dispatch time
   stamps), per-class times in AprilxStats.kernel_ms -- measurement runs only.  enable 2: the gates clock -- nothing changes in how feeds
   run (graphs replay, flights overlap) except that the feed wavefronts' gates kernels stamp their own start and end; switching back to 0
   publishes AprilxStats.gates_clock_*.  0: off. */
APRIL_EXPORT void aprilx_model_profile(AprilASRModel model, int enable);

/* state machine alone, for host-logic tests: feed (idx, max, blank) triples, receive events */
typedef struct AprilxGreedy_i *AprilxGreedy;
APRIL_EXPORT AprilxGreedy aprilx_greedy_create(AprilASRModel model, AprilRecognitionResultHandler handler, void *userdata);
/* returns 1 when the round resolved to blank; ctx_out receives the 2-token context */
APRIL_EXPORT int aprilx_greedy_step(AprilxGreedy g, int32_t idx, float max_val, float blank_val, float early_emit,
                                    size_t now_ms, int32_t *ctx_out);
APRIL_EXPORT void aprilx_greedy_finish(AprilxGreedy g);
APRIL_EXPORT void aprilx_greedy_free(AprilxGreedy g);
/* the state machine's own copy of the phrase-boosting state: attach a set (NULL = off; the state returns to the root), read the state */
APRIL_EXPORT int aprilx_greedy_set_bias(AprilxGreedy g, AprilxBias bias);
APRIL_EXPORT int aprilx_greedy_bias_state(AprilxGreedy g);
/* the state machine with search options (NULL = none); -1 on a wrong size or a value out of range */
APRIL_EXPORT int aprilx_greedy_set_search_options(AprilxGreedy g, const AprilxSearchOptions *options);
/* the state machine's own copy of the language-model node: attach a model (NULL = off; the node returns to the model's start), read the node */
APRIL_EXPORT int aprilx_greedy_set_lm(AprilxGreedy g, AprilxLm lm, float weight, float token_bonus);
APRIL_EXPORT int aprilx_greedy_lm_state(AprilxGreedy g);

/* A result handler implemented in C, for load generators and benchmarks (a Python or JNI callback costs more than
   the GPU step at thousands of sessions).  userdata -> uint64_t[6]: calls, partial, final, cant_keep_up, silence, tokens */
APRIL_EXPORT void aprilx_counting_handler(void *userdata, AprilResultType type, size_t count, const AprilToken *tokens);

/* parse + weight extraction + packing without creating any GPU object (loader tests; no sessions) */
APRIL_EXPORT AprilASRModel aprilx_model_load_host(const char *model_path);
/* fbank tables as the device sees them (window[fft_size], mel[mel][fft_size/2]); returns fft_size */
APRIL_EXPORT int aprilx_model_fbank_tables(AprilASRModel model, float *window, float *mel);

/* container-only parse (no GPU): 0 on success, otherwise -1 and a message in err */
APRIL_EXPORT int aprilx_probe_file(const char *path, char *err, size_t err_cap);

#ifdef __cplusplus
}
#endif
#endif
