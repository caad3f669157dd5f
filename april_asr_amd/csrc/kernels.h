// Device kernel interface (gfx950 only).  Launch wrappers are implemented in the
// kernels_*.hip files; engine.cc calls them on its stream.
//
// Every floating-point reduction below has a FIXED order that does not depend
// on the batch size or on the position of a row inside the batch, so a session
// stepped alone produces bit-identical state and logits to the same session
// stepped inside a batch of thousands (SURVEY.md section 7 "determinism rule").
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "vad.h"
#include "dtmf.h"
#include "tone.h"
#include "quality.h"
#include "gemm_plan.h"
#include "conv_front.h"

namespace aprilx {

// ---------------------------------------------------------------- GEMM
// out[M,N] = A[M,K] x W[K,N]  with W pre-packed for v_mfma_f32_16x16x4_f32:
//   Wp[((ntile*KB + kb)*64 + lane)*4 + j] = W[kb*16 + (lane>>4)*4 + j][ntile*16 + (lane&15)]
// so one 16-byte load per lane feeds four MFMA k-steps.
//
// Canonical summation per output element (a property of the LAYER, never of the batch):
//   K is cut into `kz` slabs, every slab into 4 contiguous chunks; a chunk is ONE in-order fp32 FMA chain
//   (that is what the MFMA computes); a slab is ((c0+c1)+c2)+c3; slabs are combined PAIRWISE in slab order
//   (balanced tree).  Two schedules produce exactly this:
//     GM_SLAB   the 4 waves of a workgroup own the 4 chunks of a slab and meet in LDS once per slab; a workgroup
//               walks zs consecutive slabs (1, 2, 4 or 8 as the batch grows), the slab tree lives in registers;
//               what is left (kz / zs planes) goes to a workspace and a row kernel finishes the same tree.
//               This is the small-batch schedule: kz x more workgroups stream the weights from HBM.
//     GM_FULLK  (kz >= 4) wave w owns the contiguous K quarter = slabs [w kz/4, (w+1) kz/4): it closes every chunk
//               chain in registers (S = ((c0+c1)+c2)+c3, then the first tree level for kz = 8), and the four waves
//               meet ONCE as (R0+R1)+(R2+R3).  No partial planes; the row work (state write, residual, bias,
//               sum of squares, slot store) runs in the GEMM epilogue.  Used as soon as output tiles alone give
//               enough workgroups.
//   fp16 one-chain rule (round 6; binary16 operands, wt == 1, on the GM_TILE / GM_PP schedules, kz = 1: gates, FFN up, the layer-major
//   halves of the gate GEMM): the sum is ONE MFMA chain over all 32-k blocks in k order -- each v_mfma_f32_16x16x32_f16 adds its 32
//   products to the running fp32 sum -- and where the y half of K ends (K0) the running sum is multiplied by the row's BasicNorm scale:
//   s * sum_y + sum_h.  EPI_XPART leaves s * sum_y, EPI_LSTM + p_add continues the chain from it.  No chunk sums: the accumulator is the
//   only register set, which is what lets GM_PP hold 256 x 128 tiles with double-buffered fragments.  Still a property of the layer:
//   every batch size, streamed or layer-major, runs the same chain.  fp32 operands keep the chunk / slab / tree form above.
// (the epilogue, prologue and mode enumerators: gemm_plan.h)
// BasicNorm never runs as a kernel.  A layer leaves y and its per-32-column sums of squares (EPI_RESID_SSQ); the consumers
// of x = y * scale(y), scale = (mean(y^2) + eps)^-1/2, fold the row scale in where it is cheapest:
//   - a GEMM over x (LSTM gates' input half, encoder_proj) runs over y and multiplies the finished partial sum by the row's
//     scale in its epilogue (`x_scale`): scale * sum_k(y_k w_k), one rounding away from sum_k((scale y_k) w_k);
//   - the residual x + h' reads y and multiplies (`r_scale`).
//     GM_TILE   (kernels_gemm_tile.hip) the four waves split the OUTPUT tile and share both operands through LDS; every wave
//               folds chunk -> slab -> tree in registers over the workgroup's zs slabs.  zs == kz: row epilogue fused;
//               zs < kz: kz / zs partial planes, finished by the row kernels exactly as for GM_SLAB.
//     GM_KW     (kernels_gemm_kw.hip, round 5) the waves split K as in GM_FULLK (eight waves: one slab each at kz = 8), but every wave's
//               activation rows arrive in full 128-byte lines through a wave-private LDS ring (no barrier in the K loop); 32 x 32 tiles.
//               The N = d_model GEMMs at a few hundred rows per launch.

//     GM_PP     (kernels_gemm_pp.hip, round 6) the fp16 gates / FFN-up GEMMs (kz = 1) from a few hundred rows per launch: 256 / 128 x 128
//               tiles on eight waves = two groups of four that run one phase apart (one group's MFMAs beside the other's DMA issue and
//               fragment reads); same chains and folds as GM_TILE.

constexpr int SSQ_COLS = 32;       // columns per sum-of-squares partial (one granule = 8 consecutive 4-column quads)

struct RowScale {                  // BasicNorm scale of a row from its sum-of-squares partials (see row_scale() in device_utils.h)
    const float *ssq = nullptr;    // [rows][groups]
    int groups = 0;                // N / SSQ_COLS
    float inv_n = 0.0f;            // 1 / N
    float eps = 0.0f;
};

// Per-slot search state (reference AprilASRSession_i: context tensor, last_emission_time_ms, the class of the
// last active token; src/april_session.h:32-73); see "greedy search on the device" below.
struct GreedyState { int32_t ctx0, ctx1; int32_t last_tok; uint32_t last_emit_ms; };

constexpr int STAMP_WORDS = 144, STAMP_ENDS = 8, STAMP_NENDS = 64, STAMP_SUBS = 72;      // layout of a gates-clock slot (GemmArgs::stamp; device_utils.h)

struct GemmArgs {
    // A operand as up to two K segments with optional row indirection (slot ids)
    const float *a0 = nullptr; int lda0 = 0; const int *aidx0 = nullptr; int K0 = 0;
    const float *a1 = nullptr; int lda1 = 0; const int *aidx1 = nullptr; int K1 = 0;
    const float *a0b = nullptr;            // AOP_TANH_ADD second addend (same ld as a0; row index aidx0b, or aidx0 when same_idx_b)
    const int *aidx0b = nullptr; int same_idx_b = 1;
    // decoder-output table (engine.h): when set, the second addend's row is table row ctx0 * ctx_vocab + ctx1 of the search
    // state of the row's slot (the index aidx0b / aidx0 would have given), i.e. a0b = the table
    const GreedyState *ctx_state = nullptr; int ctx_vocab = 0;
    int a_op = AOP_NONE;
    RowScale x_scale;                      // optional (ssq != null).  EPI_LSTM: the A-segment-0 half of the sum, ((p0+p1) * scale + p2) + p3;
                                           // EPI_SLOT_STORE: the whole sum, out = acc * scale + bias
    const void *wp = nullptr;              // packed weights (fp32, or fp16 in the same element order when wt == 1)
    int wt = 0;                            // 0: fp32 operands, v_mfma_f32_16x16x4_f32; 1: fp16 weights, A rounded to fp16 on load,
                                           //    v_mfma_f32_16x16x16_f16 with fp32 accumulation (BASELINE configs[4])
    int M = 0, N = 0, K = 0;               // N multiple of 16, K multiple of 64
    int kz = 1;                            // K slabs (power of two); canonical summation unit
    int zs = 1;                            // slabs handled per workgroup (set by launch_gemm)
    int mode = GM_SLAB;                    // set by launch_gemm
    int epi = EPI_PARTIAL;
    float *out = nullptr; int ldo = 0;     // EPI_PARTIAL: workspace [planes][m_stride][N]; others: [M][ldo] (EPI_SLOT_STORE: [slots][ldo])
    // fp16-operand engines (GM_TILE, wt == 1): activations are READ as binary16 (a0 / a1 point at binary16 rows, lda in elements)
    // and the producing epilogues leave binary16 copies beside (or instead of: out == null) the fp32 rows, same leading dimensions
    void *out16 = nullptr;                 // EPI_LSTM (u), EPI_BIAS_DSWISH (ff), EPI_HR (x + h'), EPI_RESID_SSQ (y)
    void *state16 = nullptr;               // EPI_HR: binary16 copy of the h state rows [slots][ld_state]
    int m_stride = 0;
    const float *bias = nullptr;
    float *c_state = nullptr;              // EPI_LSTM: [slots][hidden] for this layer
    const int *slot_idx = nullptr;         // EPI_LSTM / EPI_HR / EPI_SLOT_STORE: row -> slot
    int hidden = 0;
    float *state = nullptr; int ld_state = 0;     // EPI_HR: h state of this layer [slots][ld_state]
    const float *resid = nullptr; int ldr = 0;    // EPI_HR / EPI_RESID_SSQ: residual rows [M][ldr]
    RowScale r_scale;                      // EPI_HR: the residual is y * scale(y)
    float *ssq_out = nullptr;              // EPI_RESID_SSQ: [M][N / SSQ_COLS]
    const int *row_mask = nullptr;         // EPI_SLOT_STORE: optional
    const int *run_flag = nullptr;         // optional device word: the kernel returns at once unless it holds run_gen
    int run_gen = 1;
    // layer-major schedule (the encoder input of T chunks is known up front): the gate GEMM is split in two launches with the
    // SAME chains -- waves 0,1 own the input half of K, waves 2,3 the recurrent half (kz = 1, K0 = K1):
    //   wave_mask 0b0011 + EPI_XPART : P = (p0 + p1) * scale for all T x sessions rows at once
    //   wave_mask 0b1100 + EPI_LSTM + p_add : ((P + p2) + p3) + bias per time step -- bit-identical to the one-launch form
    int wave_mask = 0xF;
    const float *p_add = nullptr; int ldp = 0;
    int force_fullk = 0;                   // take the full-K plan even when it yields few workgroups (latency-bound sequential steps: one launch
                                           // instead of split-K + row kernel matters more than filling the chip)
    int zcount = 1;                        // same-shape problems sharing the launch (set by stage_gemm_z): an occupancy hint for the tile planner
    int tile_ok = 0;                       // 1 = GM_TILE may be chosen by the planner's occupancy rule (fp32 A in one K segment, N % 64 == 0, row epilogue or partial planes);
                                           // 2 = GM_TILE always (the fp16 tile path of an fp16 engine: every batch size runs the same chains)
    int asm_loop = 0;                      // != 0: hand-scheduled K loop (gemm_mainloop_asm.inc) in the fused-epilogue 64x64 fp32 tiles
    unsigned long long *trace = nullptr;   // measurement only: per-workgroup s_memtime stamps [wg][8] (wave 0, lane 0)
    // Gates launches only (EPI_LSTM; the engine's "gates clock", aprilx_model_profile(model, 2)): one slot per LAUNCH (all problems
    // of a z-batched launch point at the same one).  Every workgroup stamps real time (s_memrealtime, 10 ns) when it starts and when it has
    // finished; the last one to finish adds (latest end - earliest start) to the slot's sum and re-arms it -- the launch's duration under
    // whatever launch path is in use (graph replay), with no event packet near the kernel.  null (the product's case): two scalar branches.
    unsigned long long *stamp = nullptr;   // slot of STAMP_WORDS = 144 words (device_utils.h stamp_begin / stamp_end): [0] start, [1] classes done, [2] sum of durations (ticks), [3] launches, [8..71] end stamps, [72..135] arrival counters
    int debug = 0;                         // measurement only: 1 = skip the MFMA main loop, 2 = skip the epilogue math, 3 = all k blocks read block 0
};
void launch_gemm(const GemmArgs &g, hipStream_t s);
// Measurement (the engine's profiling mode, bench.py's roofline clock): the NEXT GEMM kernel this thread launches records its own start
// and stop into these events -- hipExtLaunchKernel puts them into the dispatch packet, i.e. the time stamps rocprofv3 reports as the
// kernel's duration, with no event packets around the kernel.  Consumed (cleared) by that launch; gemm_profile_pending() tells whether
// a launch has taken them.
void gemm_profile_next_launch(hipEvent_t start, hipEvent_t stop);
bool gemm_profile_pending();
// (internal) GM_TILE launch, called by launch_gemm / launch_gemm_z once the plan is made: tile 16 * mt rows x 16 * nt columns; dev_args != null: n z-batched problems
void launch_gemm_tile(const GemmArgs &g, int mt, int nt, const GemmArgs *dev_args, int n, hipStream_t s);
// (internal) GM_KW launch (kernels_gemm_kw.hip): tile 16 * mt rows x 16 * nt columns, all of K in the workgroup; dev_args != null: n z-batched
// problems.  gemm_kw_waves: 8 = the waves a GM_KW workgroup would use for this GEMM (operands, epilogue, chunk structure), 0 = not eligible
int gemm_kw_waves(const GemmArgs &g);
// (internal) GM_PP launch (kernels_gemm_pp.hip): tile 16 * mt (256 / 128) rows x 128 columns; dev_args != null: n z-batched problems.
// gemm_pp_ok: the operands of g fit the schedule (binary16 operands, kz = 1, LSTM / DoubleSwish / XPART epilogue, whole stages)
bool gemm_pp_ok(const GemmArgs &g, int mt);
void launch_gemm_pp(const GemmArgs &g, int mt, const GemmArgs *dev_args, int n, hipStream_t s);
// (internal) the 256 x 192 form of GM_PP (kernels_gemm_pw.hip; TilePlan.nt = 12): N a multiple of 192, EPI_LSTM / EPI_BIAS_DSWISH, all of K
bool gemm_pw_ok(const GemmArgs &g);
void launch_gemm_pw(const GemmArgs &g, const GemmArgs *dev_args, int n, hipStream_t s);
// measurement only (tools/pp_bench): enable -1 = environment default (APRIL_GM_PP), 0 / 1 = off / on; mt = 0 (planner) or pinned 16 / 8
void gemm_pp_pin(int enable, int mt);
void launch_gemm_kw(const GemmArgs &g, int mt, int nt, const GemmArgs *dev_args, int n, hipStream_t s);
// measurement only (tools/kw_bench): enable -1 = environment default (APRIL_GM_KW), 0 / 1 = off / on; mt = 0 (planner) or pinned tile rows / 16
void gemm_kw_pin(int enable, int mt);
// (internal) the recurrent GEMMs of a long feed at <= 16 rows as weight streams (kernels_recur.hip): recur_form says whether g is
// one of them (1 gates h-half + cell, 2 projection), launch_recur runs n same-shape problems (dev_args) or g itself (dev_args == null)
int recur_form(const GemmArgs &g);
void launch_recur(const GemmArgs &g, int form, const GemmArgs *dev_args, int n, hipStream_t s);
// n independent GEMMs of ONE shape (same M, N, K, kz, epilogue; any pointers) in one launch.  stage_gemm_z finalizes the
// argument blocks on the host; launch_gemm_z launches once they are in device memory at dev_args (in stream order).
// Fused-epilogue forms only (EPI_LSTM, EPI_XPART, EPI_BIAS_DSWISH, and EPI_HR / EPI_RESID_SSQ where gemm_plan says fused).
void stage_gemm_z(const GemmArgs *items, int n, GemmArgs *staged);
void launch_gemm_z(const GemmArgs *staged, int n, const GemmArgs *dev_args, hipStream_t s);
// The plan of g (gemm_plan.h): the query is built from g, capabilities included, and planned with the
// process's knobs.  A caller about to launch a row-epilogue GEMM (EPI_HR / EPI_RESID_SSQ / EPI_SLOT_STORE) asks with its fused
// form and zcount = the launch's problem count: fused -> launch it as it is; else launch its EPI_PARTIAL form, which writes
// `planes` planes, and a row kernel behind it.  For an EPI_PARTIAL g, `planes` is what its launch writes.
GemmPlan gemm_plan(const GemmArgs &g);
// The query gemm_plan builds from g: its scalar fields and the capabilities the kernel files state for it (test entries report them)
GemmQuery gemm_query(const GemmArgs &g);
// measurement only (tools/tile_bench): enable -1 = environment default, 0 / 1 = off / on; mt, zs = 0 (planner's choice) or pinned
void gemm_tile_pin(int enable, int mt, int zs);

// ---------------------------------------------------------------- row kernels (one workgroup per row; small-batch path)
enum RowMode {
    ROW_HR = 0,          // s = tree(ws); state[slot] = s; out = resid * rowscale(resid) + s
    ROW_RESID_SSQ = 1,   // y = resid + (s + bias) (resid optional); out = y; ssq partials of y
    ROW_SLOT_STORE = 2   // out[slot] = s (* rowscale, optional) + bias (rows with row_mask == 0 skipped)
};
struct RowArgs {
    int mode = ROW_HR;
    const float *ws = nullptr; int parts = 1; int m_stride = 0; int N = 0; int M = 0;
    const float *bias = nullptr;
    const float *resid = nullptr; int ldr = 0;
    RowScale r_scale;                      // ROW_HR: scale of the residual; ROW_SLOT_STORE: optional scale of the sum
    float *out = nullptr; int ldo = 0;
    const int *slot_idx = nullptr;         // row -> slot for state / slot-indexed outputs
    float *state = nullptr; int ld_state = 0;   // ROW_HR: h state of this layer
    float *ssq_out = nullptr;              // ROW_RESID_SSQ
    void *out16 = nullptr, *state16 = nullptr;   // fp16 tile engines: binary16 copies of out (ROW_HR, ROW_RESID_SSQ) and of the h state rows (ROW_HR)
    const int *row_mask = nullptr;         // ROW_SLOT_STORE
    const int *run_flag = nullptr;         // optional device word: the kernel returns at once unless it holds run_gen
    int run_gen = 1;
};
void launch_row(const RowArgs &r, hipStream_t s);
// n row problems of one mode and shape (same M, N, parts) in one launch: blockIdx.y picks the argument block (device array)
void launch_row_z(const RowArgs *host_args, int n, const RowArgs *dev_args, hipStream_t s);

// ---------------------------------------------------------------- ramp merge (engine.cc "ramp merge")
// The device words through which the layer graph of split feed k decides, once, whether its last RAMP_R macro steps also run the
// first RAMP_R macro steps of split feed k + 1 (the other flight parity).  One allocation per engine, zeroed at start.
constexpr int RAMP_R = 2;
struct RampState {
    unsigned long long ready[2];           // per parity: ramp_record(generation, m, T, hostable) of the last split feed whose front end is through
    int head_live[2];                      // per parity: 1 = the feed's first RAMP_R macro steps run in its own layer graph, 0 = a host ran them (guarded forms only, see launch_ramp_latch)
    int guest_live[2][RAMP_R][RAMP_R];     // [host parity][j - 1][t]: 1 = guest problem (layer j - 1 - t, chunk t) runs in the host's window step j
    unsigned generation;                   // split feeds made ready so far (ramp_ready_kernel is its only writer)
    unsigned hosted;                       // feeds whose head a predecessor ran (ramp_latch_kernel is its only writer)
};
// a record: generation << 32 | m << 12 | T << 4 | hostable -- ONE 8-byte word, so a reader never sees a record half written
constexpr int RAMP_MAX_M = 0xFFFFF, RAMP_MAX_T = 0xFF;
// on the front-end stream, behind the front end of a split feed of parity q (never captured: `hostable` is the host's word of the moment)
// guard: the feed's layer graph is enqueued before the latch in front of it has run, with its head steps behind head_live[q] (APRIL_RAMP_MERGE=3 / 2):
// the ready kernel arms the word and a hosting latch clears it.  0: the host enqueues the graph that fits the latch's report; head_live is not touched.
void launch_ramp_ready(RampState *rs, int q, int m, int T, int hostable, int guard, hipStream_t s);
// on the layer stream, in front of the first window step of a hosting plan of parity p and m sessions.  report: one word in pinned host
// memory, ramp_outcome_word(generation looked for, hosted) (ramp_defer.h), stored with system scope after the device words; nobody on the device waits for a reader
void launch_ramp_latch(RampState *rs, int p, int m, unsigned long long *report, int guard, hipStream_t s);

// ---------------------------------------------------------------- greedy search on the device
// Per-slot search state (reference AprilASRSession_i: context tensor, last_emission_time_ms, the class of the
// last active token; src/april_session.h:32-73).  The host keeps the token list and runs the callbacks; the
// device keeps what the NEXT network call depends on, so a chunk needs no host decision.
// One joiner round of one session.  flags: 1 = valid (the round ran), 2 = resolved to blank, 4 = context changed
struct StepRecord { int32_t idx; float max_val; float blank_val; uint32_t flags; };
// Side record of one joiner round of a session that asked for confidences (aprilx_session_set_confidence):
// log-sum-exp of the round's logits, the blank's logit and the n_alt best non-blank ids with their logits (logit descending, lower
// id first on ties; [0] is StepRecord.idx / max_val bit for bit).  Unused entries hold id -1 / logit 0, so a record is a fixed
// function of (row, K).  Written by decide_kernel beside the StepRecord, in a ring of its own with the same indexing.
constexpr int kConfMaxAlt = 8;
struct ConfRecord { float lse; float blank_val; int32_t n_alt; uint32_t reserved; int32_t alt_id[kConfMaxAlt]; float alt_logit[kConfMaxAlt]; };
static_assert(sizeof(ConfRecord) == 80, "ConfRecord is 20 x 32 bit");
enum { REC_VALID = 1, REC_BLANK = 2, REC_CTX = 4 };
enum TokClassBits { TKC_WORD_START = 1, TKC_SENT_END = 2, TKC_COMMA = 4, TKC_DOT = 8, TKC_DIGIT_START = 16 };

// Phrase boosting (bias.h): one bias set on the device -- the effective token edges of every trie state, CSR
struct BiasDesc { const int32_t *state_off = nullptr, *edge_tok = nullptr, *edge_next = nullptr; const float *edge_bonus = nullptr; int32_t n_states = 0, flags = 0; };      // flags: BiasSet::flags (kBiasStrict)

// Per-session search options: one entry per slot.  endpoint_ms == 0: the slot's session has none (the decision
// runs its unchanged lines); else the silence that ends an utterance in ms (200 .. 60000) and the blank penalty p (bl' = bl - p).
struct SearchOpt { uint32_t endpoint_ms; float blank_penalty; };
static_assert(sizeof(SearchOpt) == 8, "SearchOpt is 2 x 32 bit");

// Text-corpus language model (lm.h): one model on the device -- the CSR of the back-off automaton and the token
// text table --, and one entry per slot: the slot's model (index into the descriptor table, -1 = none), weight w, per-token bonus b and
// the model's start node (what the end-of-flush reset writes).
struct LmDesc {
    const int32_t *node_off = nullptr, *back = nullptr, *arc_next = nullptr, *tok_off = nullptr;
    const float *bow = nullptr, *arc_logp = nullptr;
    const uint8_t *arc_byte = nullptr, *tok_bytes = nullptr;
    int32_t n_nodes = 0, start = 0; float unk_logp = 0.0f; int32_t reserved = 0;
};
struct LmSlot { int32_t model; float w, b; int32_t start; };
static_assert(sizeof(LmSlot) == 16, "LmSlot is 4 x 32 bit: one load");

struct DecEmbedParams {
    const float *emb = nullptr;            // [vocab][d]
    const float *conv_w = nullptr;         // [d][d/groups][context]
    const float *conv_b = nullptr;         // optional [d]
    int d = 0, groups = 0, context = 0, vocab = 0;
};

// Masked arg-max over the joiner logits + the blank / non-blank decision of src/april_session.c:306-429 that
// drives the data path (context push, decoder re-run, silence reset) + the decoder front end for rows whose context
// changed.  One workgroup per row.
struct DecideArgs {
    const float *ws = nullptr; int parts = 1; int m_stride = 0; int N = 0; int M = 0;   // logits = tree(ws) + bias
    int n_valid = 0;                       // vocabulary size (<= N)
    const float *bias = nullptr;
    int blank = 0;
    float early_emit = 0.0f;               // 1.0 in the first round of a chunk, 0.0 afterwards (:449-454)
    const int *slot_idx = nullptr;         // row -> slot
    const int *now_ms = nullptr;           // row -> session time of this chunk
    int *active = nullptr;                 // row -> `gen` while the row is still searching in this chunk (in/out; round 0 treats every row as active)
    int gen = 1;                           // generation of this chunk inside the step (1 for a one-chunk step, t + 1 in a layer-major step)
    int rec_slot = 0;                      // record index of this round inside the step's record block (chunk * 3 + round)
    int *dirty = nullptr;                  // row -> context changed in this round (out; the decoder projection's row mask)
    const uint8_t *tok_class = nullptr;    // [vocab] TokClassBits
    GreedyState *state = nullptr;          // [slots]
    StepRecord *rec = nullptr;             // [M] records of this round, or null (see rec_ring)
    StepRecord *rec_ring = nullptr;        // records go to rec_ring[*rec_off + round * M + row] when rec == null
    const int *rec_off = nullptr; int round = 0;
    float *logits_dump = nullptr;          // optional [M][n_valid]
    DecEmbedParams dec;
    float *de_out = nullptr; int ld_de = 0;   // relu(conv(emb[ctx])) rows for dirty rows
    // round flags (device words, zeroed by the advance kernel): run[r] == gen: some row still searches in round r (r > 0),
    // rerun[r] == gen: some row's context changed in round r.  A round nobody needs costs three empty launches.
    int *run_flags = nullptr;              // [3]
    int *rerun_flags = nullptr;            // [3]
    // confidences (kernels_confidence.inc): null / 0 unless a session of the engine opted in.  conf_k: per-slot K (0 = off);
    // the side record goes to conf_ring at the StepRecord's ring index, or to conf[row] with conf_k_all alternatives (tests)
    const uint8_t *conf_k = nullptr;       // [slots]
    ConfRecord *conf_ring = nullptr;
    ConfRecord *conf = nullptr; int conf_k_all = 0;
    // phrase boosting (kernels_bias.inc): null unless a session of the engine opted in.  bias_set: per-slot index into bias_desc
    // (-1 = none); bias_state: per-slot trie state (0 = root), read and written by the decision beside `state`
    const int32_t *bias_set = nullptr;     // [slots]
    int32_t *bias_state = nullptr;         // [slots]
    const BiasDesc *bias_desc = nullptr;
    // search options: null unless a session of the engine opted in
    const SearchOpt *opt = nullptr;        // [slots]
    // language model (kernels_lm.inc): null unless a session of the engine opted in (then the three bias tables
    // exist as well: the LM forms are built on the BIAS forms).  Last in the struct: the other forms' argument offsets stay what they were
    const LmSlot *lm_slot = nullptr;       // [slots]
    int32_t *lm_state = nullptr;           // [slots] node ids, read and written by the decision beside bias_state
    const LmDesc *lm_desc = nullptr;
};
void launch_decide(const DecideArgs &a, hipStream_t s);

// Decoder front end for listed slots, context taken from the device state.  op 1 first applies the end-of-flush
// reset (last token forgotten; context cleared to [blank, blank] unless it already starts with blank,
// src/april_session.c:296-301,561-563).
struct DecRowsArgs {
    const int *slot_idx = nullptr; int M = 0;
    int op = 0; int blank = 0;
    GreedyState *state = nullptr;
    DecEmbedParams dec;
    float *de_out = nullptr; int ld_de = 0;
    int32_t *bias_state = nullptr;         // [slots] or null: op 1 also returns the slot's phrase-boosting state to the root
    const LmSlot *lm_slot = nullptr;       // [slots] or null: op 1 also returns the slot's language-model state to its model's start node
    int32_t *lm_state = nullptr;
};
void launch_dec_rows(const DecRowsArgs &a, hipStream_t s);

// debug / parity entry point: decoder front end with explicit contexts
struct DecEmbedArgs {
    DecEmbedParams dec;
    const int *ctx = nullptr;              // [M][context]
    int M = 0;
    float *out = nullptr; int ldo = 0;
};
void launch_dec_embed(const DecEmbedArgs &a, hipStream_t s);

// start of a step inside a launch chain whose arguments are fixed (hipGraph): fetches the step's index block
// (n_arrays arrays of `len[a]` ints: slots | ring tails | session times | row slots) from the pinned host ring through the
// device step counter
struct AdvanceArgs {
    const int *host_ring = nullptr;        // pinned, device-readable
    const int *host_step_off = nullptr;    // pinned: [step] -> offset of the step's block in host_ring
    const int *host_rec_off = nullptr;     // pinned: [step] -> offset of the step's records in the record ring
    int *counter = nullptr;                // device: next step (runs on for the life of the engine; table index = counter & index_mask)
    int index_mask = 0x7fffffff;
    int *dst = nullptr; int dst_stride = 0;   // device: [n_arrays][dst_stride]
    int n_arrays = 3; int len[4] = {0, 0, 0, 0};
    int *rec_off = nullptr;                // device: record offset of the current step
    int *flags = nullptr; int n_flags = 0; // device: zeroed
};
void launch_advance(const AdvanceArgs &a, hipStream_t s);

// slot reset (aas_free / session create): recurrent state, encoder/decoder outputs and the search state of one slot
struct ZeroSlotArgs {
    float *h = nullptr, *c = nullptr; int n_layers = 0; size_t slots = 0; int d_model = 0, hidden = 0;
    float *eout = nullptr, *dout = nullptr; int joiner = 0;
    GreedyState *state = nullptr; int blank = 0;
    int slot = 0;
    void *h16 = nullptr;                   // fp16 tile engines: the binary16 copy of h, zeroed too
    int n_list = 0; int list[64] = {0};    // n_list > 0: the listed slots in ONE launch (grid.y), `slot` unused
};
void launch_zero_slot(const ZeroSlotArgs &a, hipStream_t s);

// Session snapshot / restore: one launch moves the per-slot state of n sessions between the engine's arrays and a
// staging buffer that holds one device block per session.  A block is the concatenation of the arrays below at 16-byte aligned offsets:
// array i contributes `layers` rows of row_bytes bytes (row l of slot s at base + s * slot_stride + l * layer_stride) at block offset off.
// The last array may be the feature ring (ring != 0): its row count comes from the session's record, row r of the block is ring row
// (tail + r) % ring_frames.  Arrays whose bit is clear in the record's mask are skipped (gather leaves zeros, scatter leaves the slot's).
constexpr int kSnapMaxArrays = 10;
struct SnapArray { char *base = nullptr; unsigned long long slot_stride = 0, layer_stride = 0; uint32_t layers = 0, row_bytes = 0, off = 0, ring = 0; };
struct SnapRec { int32_t slot = 0, tail = 0, rows = 0, tgt_tail = 0; uint32_t mask = 0, block_bytes = 0; unsigned long long stage_off = 0; };
static_assert(sizeof(SnapRec) == 32, "uploaded as bytes");
struct SnapArgs {
    SnapArray arr[kSnapMaxArrays]; int n_arr = 0;
    const SnapRec *recs = nullptr; int n = 0;      // device
    char *stage = nullptr;                         // device: block i at stage + recs[i].stage_off
    int ring_frames = 0;
    int scatter = 0;                               // 0: arrays -> staging (ring rows from tail); 1: staging -> arrays (ring rows to tgt_tail)
    int vec = 4;                                   // bytes per lane and access: 16 where every base, stride, width and offset is a multiple of 16, else 4
    uint32_t max_block = 0;                        // the largest block of the call (sizes the grid)
};
void launch_snapshot_copy(const SnapArgs &a, hipStream_t s);

// Search bookkeeping of one BLOCK of time steps of a layer-major step, so that the search's launch chain has arguments that do
// not depend on the block (one captured graph serves every block): the block's session times and encoder-output row numbers
// are copied to fixed places, the record offset of the block is derived from the step's, the round flags are cleared.
struct BlockSetupArgs {
    const int *now_src = nullptr; int *now_dst = nullptr;     // [count] session times of the block's rows
    int *rows_dst = nullptr; int row0 = 0; int count = 0;     // rows_dst[i] = row0 + i
    const int *rec_off_step = nullptr; int *rec_off_block = nullptr; int rec_add = 0;
    int *flags = nullptr; int n_flags = 0;
};
void launch_block_setup(const BlockSetupArgs &a, hipStream_t s);

// ---------------------------------------------------------------- encoder front (conv 1+2, im2col for conv 3)
struct ConvEmbedArgs {
    const float *ring = nullptr;           // [slots][ring_frames][mel]
    int ring_frames = 0, mel = 0, seg = 0;
    const int *slot_idx = nullptr;         // row -> slot
    const int *ring_tail = nullptr;        // row -> first ring row of the chunk
    const float *w[3] = {nullptr, nullptr, nullptr};
    const float *b[3] = {nullptr, nullptr, nullptr};
    int ch[3] = {0, 0, 0};
    int ch1_per_group = 0;                 // second-conv channels per workgroup (grid.y = ch[1] / this)
    int stride[3] = {1, 2, 2};
    float *out = nullptr; int ldo = 0;     // im2col rows of the third conv: [M * f_out][ldo], k = ci*9 + i*3 + j
    int M = 0;
    const float *x_direct = nullptr;       // debug path: x given as [M][seg][mel] instead of the ring
    const float *w0t = nullptr, *w1t = nullptr;      // optional: the first two convs' weights transposed (launch_conv_weight_transpose): [9][ch0], [ch0 * 9][ch1] -- the many-chunk form needs them
};
void launch_conv_embed(const ConvEmbedArgs &a, hipStream_t s);
// which form launch_conv_embed runs: 1 = the many-chunk form (one workgroup per chunk, all channels), 0 = the grouped form.  The
// second conv's channels per workgroup of the grouped form are conv_ch1_per_group (conv_front.h) of ch[1].
int conv_embed_form(const ConvEmbedArgs &a);
void launch_conv_weight_transpose(const float *w0, const float *w1, int c0, int c1, float *w0t, float *w1t, hipStream_t s);

// fp32 -> fp16 (round to nearest even), elementwise; used once at load for the fp16 weight copies
void launch_cvt_f16(const float *src, void *dst, size_t n, hipStream_t s);

// fp32 packed weights (16-k blocks, kernels.h top) -> binary16 in the order of v_mfma_f32_16x16x32_f16's B fragment:
//   dst[((ntile * (K / 32) + kb) * 64 + lane) * 8 + j] = W[kb * 32 + (lane >> 4) * 8 + j][ntile * 16 + (lane & 15)]
// (one 16-byte read per lane and 32-k block; K a multiple of 32)
void launch_repack_x32(const float *src_packed, void *dst, int K, int N, hipStream_t s);

// ---------------------------------------------------------------- fbank
struct FbankTables {                       // device pointers
    const float *window = nullptr;         // [padded]
    const double *tw[16] = {nullptr};      // per factor twiddles (pocketfft layout)
    const double *tws[16] = {nullptr};     // factors above 5: the generic pass's roots of unity (cos, sin)(2 pi i / ip)
    int fct[16] = {0}; int nfct = 0;
    const float *mel = nullptr;            // [nbins][padded/2]
    const int *mel_lo = nullptr;           // [nbins] first non-zero fft bin
    const int *mel_hi = nullptr;           // [nbins] one past the last non-zero fft bin
    int padded = 0, nbins = 0;
};
struct FbankFrameDesc { int32_t slot; int32_t ring_row; int32_t pcm_off; };   // pcm_off < 0: padding row log(kEps)
struct FbankArgs {
    FbankTables t;
    const int16_t *pcm = nullptr;          // staged samples
    const FbankFrameDesc *desc = nullptr;
    int n_frames = 0;
    float *ring = nullptr; int ring_frames = 0;
    float pad_value = 0.0f;
};
void launch_fbank(const FbankArgs &a, hipStream_t s);

// ---------------------------------------------------------------- resample (sessions with an input rate of their own)
// Input-rate PCM16 -> model-rate PCM16 into the staging buffer fbank_kernel reads (FbankFrameDesc::pcm_off), by the contract of
// resample.h: y[j] = sat16(round_half_even(sum_i tap[p][i] x[k0 - K + 1 + i])), one fp32 FMA chain in increasing i, x = 0
// outside the staged span (the host stages every sample of the segment that a written output needs).  One descriptor per
// resampled window and segment; outputs j < 0 and j >= out_end are written as 0 (the flush zeros behind a closed segment).
struct ResampleDesc {
    const float *taps = nullptr;           // phase table [L][ldt] (device; uploaded once per conversion and engine)
    int64_t in_base = 0;                   // segment input index of the first staged sample
    int64_t out_first = 0;                 // segment output index of the first output
    int64_t out_end = 0;                   // segment output end
    int32_t in_off = 0, in_n = 0;          // staged input span: staging offset, samples
    int32_t out_dst = 0, out_cnt = 0;      // model-rate staging offset, outputs
    int32_t L = 1, M = 1, K = 0, ldt = 0;
};
struct ResampleArgs {
    const int16_t *in = nullptr;           // staging buffer (input spans)
    int16_t *out = nullptr;                // staging buffer (model-rate regions)
    const ResampleDesc *desc = nullptr;
    int n_desc = 0;
    int max_blocks = 0;                    // max over descriptors of ceil(out_cnt / kResampleBlock)
    int lds_floats = 0;                    // max over descriptors of resample_lds_floats(L, M, K)
};
void launch_resample(const ResampleArgs &a, hipStream_t s);

// ---------------------------------------------------------------- decode (sessions with an input format)
// Raw bytes -> int16 into the staging buffer resample_kernel and fbank_kernel read, by the contract of input_format.h: one int16 per
// audio frame of `channels` interleaved values.  One descriptor per staged span: outputs [0, n_src) are decoded from the frames that
// start at raw byte src_off, outputs [n_src, out_cnt) are written as 0 (the flush zeros behind a segment).  CONTRACT: src_off is a
// multiple of 4 (the host starts every raw span on a 4-byte boundary of the raw region, whose base is 16-byte aligned), so a frame's
// values are naturally aligned -- 2 bytes for S16, 4 for F32 -- and every load is an aligned load of one value.
constexpr int kDecodeBlock = 256;
struct DecodeDesc {
    int64_t src_off = 0;                   // byte offset of the first frame inside the raw region
    int32_t dst = 0;                       // int16 staging offset of the first output
    int32_t out_cnt = 0, n_src = 0;        // outputs written, of which decoded
    uint8_t encoding = 0, channels = 1; int8_t channel = 0;
    uint8_t dst_in = 0;                    // (host only) dst counts from the start of the input-rate spans: Engine::fbank adds the model-rate samples
};
struct DecodeArgs {
    const uint8_t *raw = nullptr;          // raw region
    int16_t *out = nullptr;                // staging buffer
    const DecodeDesc *desc = nullptr;
    int n_desc = 0;
    int max_blocks = 0;                    // max over descriptors of ceil(out_cnt / kDecodeBlock)
};
void launch_decode(const DecodeArgs &a, hipStream_t s);

// ---------------------------------------------------------------- voice activity (sessions that opted in; contract in vad.h)
// One workgroup per descriptor: one session's contiguous run of real feature rows of this pass (rows wrap modulo ring_frames), in
// frame order.  The descriptor carries the session's plan (32 bytes: no per-slot plan table to keep in step), and VAD_RESET when the
// run is the first one after the options were set or a flush completed: the kernel then starts from the reset state instead of the
// slot's record.  One byte per frame goes to out[out_off + i], the slot's 64-byte record is read once and written once.
constexpr int kVadBlock = 256, kVadTile = 256;           // lanes per workgroup; frames whose energies one LDS tile holds
enum : int32_t { VAD_RESET = 1 };
struct VadDesc {
    int32_t slot = 0, first_row = 0, n = 0, out_off = 0;  // ring rows (first_row + i) % ring_frames, i < n <= ring_frames
    int32_t flags = 0, reserved[3] = {0, 0, 0};
    VadPlan plan;
};
static_assert(sizeof(VadDesc) == 64, "staged behind the decode descriptors, 16-byte aligned");
struct VadArgs {
    const float *ring = nullptr; int ring_frames = 0, nbins = 0;      // [slots][ring_frames][nbins]
    const VadDesc *desc = nullptr; int n_desc = 0;
    VadState *state = nullptr;             // [slots]
    uint8_t *out = nullptr;                // the pass's bytes
    float *energy = nullptr;               // (tests) step 1's e of every frame, indexed like out; or null
};
void launch_vad(const VadArgs &a, hipStream_t s);

// ---------------------------------------------------------------- DTMF (sessions that opted in; contract in dtmf.h)
// One descriptor per run of consecutive real frames of a session in this pass: frame i of the run is frame descriptor first + i of the
// SAME pass (its pcm_off: no sample is staged twice), one byte per frame goes to out[out_off + i].  The descriptor carries the session's
// plan; the kernel keeps no state.  One wave per frame, kDtmfBlock / 64 waves per workgroup, a wave walks every (waves of its
// descriptor)-th frame of the run.
constexpr int kDtmfBlock = 256, kDtmfWaveFrames = 4, kDtmfMaxBlocks = 64;      // lanes per workgroup; frames a wave walks before another workgroup is worth it
struct DtmfDesc {
    int32_t first = 0, n = 0, out_off = 0, reserved[3] = {0, 0, 0};
    DtmfPlan plan;
};
static_assert(sizeof(DtmfDesc) == 64, "staged behind the VAD descriptors, 16-byte aligned");
struct DtmfArgs {
    const int16_t *pcm = nullptr;          // staged samples
    const FbankFrameDesc *frames = nullptr;
    const DtmfDesc *desc = nullptr; int n_desc = 0;
    int max_n = 0;                         // max over descriptors of n
    const float *tables = nullptr; int wd = 0;      // [16][wd] (dtmf_make_tables); every descriptor's plan.Wd is wd
    uint8_t *out = nullptr;                // the pass's bytes
    float *powers = nullptr;               // (tests) P[0..8) and E of every frame, [.][9] indexed like out; or null
};
void launch_dtmf(const DtmfArgs &a, hipStream_t s);
// (tests) the decision alone on GIVEN rows of P[0..8), E: codes_out[i] = dtmf_decide(plan, powers9 + 9 i)
void launch_dtmf_decide(const DtmfPlan &plan, int n, const float *powers9, uint8_t *codes_out, hipStream_t s);

// ---------------------------------------------------------------- tones (sessions that opted in; contract in tone.h)
// One descriptor per run of consecutive real frames of a session in this pass, laid out as DtmfDesc: frame i of the run is frame
// descriptor first + i of the SAME pass, its record (two uint16, four bytes) goes to out + 4 (out_off + i).  The descriptor carries the
// session's plan; the kernel keeps no state.  One wave per workgroup, kToneWaveFrames consecutive frames of a run per wave.
constexpr int kToneBlock = 64, kToneWaveFrames = 4, kToneBins = 8;      // lanes per workgroup; frames a wave carries; bins per walk of the rows
struct ToneDesc {
    int32_t first = 0, n = 0, out_off = 0, reserved = 0;
    TonePlan plan;
};
static_assert(sizeof(ToneDesc) == 64, "staged behind the DTMF descriptors, 16-byte aligned");
struct ToneArgs {
    const int16_t *pcm = nullptr;          // staged samples
    const FbankFrameDesc *frames = nullptr;
    const ToneDesc *desc = nullptr; int n_desc = 0;
    int max_n = 0;                         // max over descriptors of n
    const float *tables = nullptr; int w = 0, f = 0;      // [2 f][w] (tone_make_tables); every descriptor's plan.W is w and plan.F is f
    uint32_t *out = nullptr;               // the pass's records (4-byte aligned)
    float *powers = nullptr;               // (tests) P[0..f) and E of every frame, [.][f + 1] indexed like out; or null
};
void launch_tone(const ToneArgs &a, hipStream_t s);
// (tests) the decision alone on GIVEN rows of P[0..F), E: records_out[i] = tone_decide(plan, powers + (F + 1) i)
void launch_tone_decide(const TonePlan &plan, int n, const float *powers, uint32_t *records_out, hipStream_t s);

// ---------------------------------------------------------------- line quality (sessions that opted in; contract in quality.h)
// One descriptor per run of consecutive real frames of a session in this pass, laid out as DtmfDesc: frame i of the run is frame
// descriptor first + i of the SAME pass, its record (eight uint32, 32 bytes) goes to out + 8 (out_off + i).  The descriptor carries the
// session's clip level; the kernel keeps no state.  One wave per frame, kQualityBlock / 64 waves per workgroup, a wave walks every
// (waves of its descriptor)-th frame of the run.
constexpr int kQualityBlock = 256, kQualityLanes = 64, kQualityWaveFrames = 4, kQualityMaxBlocks = 64;      // lanes per workgroup and wave; frames a wave walks before another workgroup is worth it
struct QualityDesc {
    int32_t first = 0, n = 0, out_off = 0, clip_level = 32767;
};
static_assert(sizeof(QualityDesc) == 16, "staged behind the tone descriptors, 16-byte aligned");
struct QualityArgs {
    const int16_t *pcm = nullptr;          // staged samples
    const FbankFrameDesc *frames = nullptr;
    const QualityDesc *desc = nullptr; int n_desc = 0;
    int max_n = 0;                         // max over descriptors of n
    int hop = 0;                           // H: samples of a frame the record covers (at most the staged frame's length)
    uint32_t *out = nullptr;               // the pass's records (16-byte aligned)
};
void launch_quality(const QualityArgs &a, hipStream_t s);

}  // namespace aprilx
