// Per-GPU engine: packed weights + slot-indexed persistent session state in HBM
// and the batched step functions that replace the three ORT Run() calls of the
// reference (src/april_session.c:131-179) and its per-session fbank
// (src/fbank.c:174-306).
//
// HBM layout (fp32, row-major):
//   h      [L][slots][d_model]      LSTM projected hidden state      (reference h tensor (L,1,d))
//   c      [L][slots][hidden]       LSTM cell state                  (reference c tensor (L,1,H))
//   ring   [slots][ring_frames][mel]  log-mel feature ring           (reference OnlineFBank ring)
//   eout   [slots][joiner]          projected encoder output of the last chunk
//   dout   [slots][joiner]          projected decoder output of the current token context
//   gstate [slots]                  greedy-search state (token context, last emission time, last token)
// plus per-step work buffers sized for `max_batch` rows.  State never leaves HBM
// between feed calls; per joiner round 16 bytes per session come back (StepRecord), once per flight, plus one side record
// (ConfRecord, 80 bytes) per row of a session that asked for confidences (aprilx_session_set_confidence).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdint>
#include <deque>
#include <array>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>
#include "bias.h"
#include "lm.h"
#include "fbank_tables.h"
#include "resample.h"
#include "input_format.h"
#include "kernels.h"
#include "host_pool.h"
#include "ramp_defer.h"
#include "slot_queue.h"
#include "staging_layout.h"
#include "pass_layout.h"
#include "model_loader.h"

namespace aprilx {

// Packed, device-layout weights as ONE contiguous blob (so they can be broadcast with a
// single collective and uploaded with a single copy).  Offsets are in floats.
struct PackedLayout {
    NetDims dims;
    size_t conv_w[3], conv_b[3];
    int k3 = 0;                              // K of the third conv as a GEMM (conv_ch[1]*9 rounded up to 64)
    size_t w_embed, b_embed;
    struct Layer { size_t wg, bg, whr, wff1, bff1, wff2, bff2; };
    std::vector<Layer> layers;
    size_t w_encproj, b_encproj, emb, dec_conv, dec_conv_b, w_decproj, b_decproj, w_out, b_out;
    size_t total = 0;
    int vocab_pad = 0;                       // joiner N padded to 16
    bool has_dec_conv_b = false;
    std::vector<float> norm_eps;             // [L]
    float embed_eps = 0;
};
void plan_layout(const NetDims &d, bool has_dec_conv_b, PackedLayout &L);
// (offset, count) of every MFMA-packed Linear / LSTM weight matrix inside the blob, in blob order: the sections that get
// binary16 copies in fp16-operand mode and are stored as binary16 in the fp16 cache file
std::vector<std::pair<size_t, size_t>> gemm_sections(const PackedLayout &L);
// fills `blob` (L.total floats) from the neutral host weights
void pack_weights(const HostModel &m, PackedLayout &L, std::vector<float> &blob);

// Process-wide lock between graph captures and everything that uses the LEGACY stream or allocates (hipMemcpy, hipMemset, hipMalloc,
// hipFree ...).  While any stream of the process is being captured, such a call from another thread fails
// ("operation would make the legacy stream depend on a capturing blocking stream" / hipErrorStreamCaptureUnsupported) and poisons the
// capture -- measured on ROCm 7.2 also for non-blocking streams and relaxed-mode captures -- and client threads make such calls: a
// second model being loaded, aprilx_session_read_frames / aprilx_session_context on an idle session, blob export.  Captures hold the
// lock for their few milliseconds, the legacy-stream users for theirs.  Recursive: the debug entry points hold it and may capture.
std::recursive_mutex &hip_legacy_mutex();
struct HipLegacyLock { std::lock_guard<std::recursive_mutex> g; HipLegacyLock() : g(hip_legacy_mutex()) {} };

struct EngineConfig {
    int device = 0;
    int max_slots = 4096;
    int max_batch = 2048;
    int precision = 0;                       // 0: fp32 GEMMs; 1: fp16 weights + fp16-rounded activations, fp32 accumulate (APRIL_PRECISION=f16)
};

struct KernelTiming { double ms = 0; long launches = 0; };

// One family of captured launch chains: key -> instantiated graph, with a capacity.  A full family is emptied as a whole (its owner first drains the streams that may
// still run one of its execs).  use() counts how often a batch shape has come by, for the families that capture at the SECOND use: a capture costs milliseconds.
struct GraphCache {
    using Key = std::array<int, 3>;          // {rows m (negated: built under the gates clock), chunks T / block length, flight parity * 8 + part}
    const char *name; size_t cap;
    bool full() const { return map_.size() >= cap; }
    hipGraphExec_t find(const Key &k) const { auto it = map_.find(k); return it == map_.end() ? nullptr : it->second; }
    void insert(const Key &k, hipGraphExec_t g) { map_[k] = g; }
    int use(int m, int T = 0) { return ++uses_[std::make_pair(m, T)]; }
    void clear();                            // destroys every exec and forgets the use counts (engine.cc); one INFO line
    std::map<Key, hipGraphExec_t> map_; std::map<std::pair<int, int>, int> uses_;
};

// Ramp merge, the pure part: which problems of the NEXT feed's first R macro steps the last R macro steps of a feed of T chunks over
// L layers can hold.  Window step j (1..R) is own macro step L + T - 1 - R + j and takes the guests of the next feed's step j:
// (layer j - 1 - t, chunk t), t < j.  Empty when the window would reach into the feed's own head or a guest would meet a layer
// before the feed's last chunk has left it (L <= 2 R), or when own + guest problems exceed `max_problems` in some step.
struct RampStep { int macro = 0, own = 0; std::vector<std::pair<int, int>> guests; };      // guests: (layer, chunk)
std::vector<RampStep> ramp_window(int L, int T, int R, int max_problems = 3);

// One per-slot opt-in table on the engine's side ("life cycle"): device array + pinned host mirror.  Nothing exists
// until alloc() -- the decision launches carry a null pointer until then --, and the device pointer never changes afterwards (captured
// graphs hold it).  The stepping thread writes the mirror and uploads the WHOLE table, stream-ordered ahead of the flight's steps.
template <typename T> struct DeviceTable {
    T *d = nullptr, *h = nullptr; size_t n = 0;
    bool on() const { return h != nullptr; }
    void alloc(size_t count, const T &off);         // every entry `off` (legacy lock held by the caller or taken inside: recursive)
    void upload(hipStream_t st) const;
    void release();
};

// The front-end passes that ride along with one Engine::fbank() call (default: none, and fbank() issues exactly the launches it always did).
// All arrays are the caller's and are read during the call only.
struct FrontPass {
    // Resampled sessions (aprilx_session_set_input_rate): a PCM part with a null pointer only RESERVES its model-rate region; the input-rate
    // spans `in_parts` (n_in samples) follow the model-rate regions in the same staging buffer, and the n_rs descriptors (in_off relative to
    // the first input span, out_dst absolute; rs_specs[i] is descriptor i's conversion, whose device table fbank() fills in) fill the
    // reserved regions in one resample launch before the fbank launch.
    int n_rs = 0; ResampleDesc *rs = nullptr; const ResampleSpec *const *rs_specs = nullptr;
    const std::pair<const int16_t *, size_t> *in_parts = nullptr; size_t n_in_parts = 0, n_in = 0;
    // Sessions with an input format (aprilx_session_set_input_format): their raw bytes `raw_parts` (n_raw bytes; every span starts on a
    // 4-byte boundary, `raw_parts` carries the padding as null parts) form a third staged region behind the two int16 ones.  The n_dc
    // descriptors (src_off relative to that region; dst absolute, or counted from the input-rate spans when dst_in is set) fill int16
    // regions that were only reserved, in one decode launch before the resample and the fbank launch.
    int n_dc = 0; const DecodeDesc *dc = nullptr;
    const std::pair<const uint8_t *, size_t> *raw_parts = nullptr; size_t n_raw_parts = 0, n_raw = 0;
    // The frame observers (voice activity, DTMF, tones, line quality), indexed by Observer: the descriptors of the
    // observer's runs and the frames they cover in all.  Each writes one record per frame into its part of the block fbank() returns
    // (pass_layout.h); a descriptor's out_off counts records from the start of its observer's part.  A VAD descriptor names ring rows:
    // vad_kernel runs right behind the fbank launch.  The others read staged samples (`first` indexes the frame descriptors of this call):
    // dtmf_kernel, tone_kernel and quality_kernel run behind the resample launch, in front of the fbank launch.
    struct Observed { int n = 0; const void *desc = nullptr; size_t frames = 0; } obs[OBS_COUNT];
    int quality_hop = 0;                       // H of the plans behind the quality descriptors: the model's frame shift in samples
    static constexpr Observer observer_of(const VadDesc *) { return OBS_VAD; }
    static constexpr Observer observer_of(const DtmfDesc *) { return OBS_DTMF; }
    static constexpr Observer observer_of(const ToneDesc *) { return OBS_TONE; }
    static constexpr Observer observer_of(const QualityDesc *) { return OBS_QUALITY; }
    template <typename Desc> void observe(const Desc *d, size_t n, size_t frames) { obs[observer_of(d)] = Observed{(int)n, d, frames}; }
    template <typename Desc> const Desc *descs() const { return static_cast<const Desc *>(obs[observer_of((const Desc *)nullptr)].desc); }
};

// One call of the decision kernel on GIVEN rows (the parity tests' entry point, Engine::debug_decide): slots 0..n-1, row i = slot i.
struct DecideRequest {
    int n = 0, op = 0;                         // op 0: one decide_kernel round; 1: the end-of-flush reset
    const float *logits = nullptr;             // [n][vocab] (op 0)
    float early_emit = 1.0f; const int *now_ms = nullptr /* null: 0 */; int round = 0;
    int32_t *state_io = nullptr;               // [n] GreedyState in and out; null: the slots' reset state
    StepRecord *rec_out = nullptr;             // [n] (op 0)
    const BiasSet *set = nullptr; int32_t *bias_state_io = nullptr;      // tables of their own for the call: row i uses the set from trie state bias_state_io[i], or none when that is -1
    const SearchOpt *opts = nullptr;           // a table of its own likewise: opts[i] on row i (endpoint_ms 0 = a row without options)
    const LmSet *lm = nullptr; int32_t *lm_state_io = nullptr; float lm_weight = 0.0f, lm_bonus = 0.0f;      // likewise: row i walks the model from node lm_state_io[i], or has none when that is -1
    int conf_k = 0; ConfRecord *conf_out = nullptr;                      // conf_k > 0: the side records of the rows with conf_k alternatives
    // the arguments the aprilx_run_decide* family shares
    static DecideRequest round_of(int n, int op, const float *logits, float early_emit, const int32_t *now_ms, int round, int32_t *state_io, void *records_out)
    {
        DecideRequest q;
        q.n = n; q.op = op; q.logits = logits; q.early_emit = early_emit; q.now_ms = (const int *)now_ms; q.round = round; q.state_io = state_io; q.rec_out = (StepRecord *)records_out;
        return q;
    }
};

class Engine {
public:
    Engine(const EngineConfig &cfg, const PackedLayout &layout, const float *blob_host, const float *blob_device,
           const ModelParams &params, const FbankHostTables &ft, const std::vector<uint8_t> &tok_class);
    ~Engine();

    int device() const { return cfg_.device; }
    int max_batch() const { return cfg_.max_batch; }
    int max_slots() const { return cfg_.max_slots; }
    int ring_frames() const { return ring_frames_; }
    const NetDims &dims() const { return L_.dims; }
    hipStream_t stream() const { return stream_; }
    const float *weights_device() const { return w_; }
    float *weights_mut() { return w_; }        // load time only: the constructor leaves the weights unset when it is given no blob
    void finish_weights();                     // after the weights are in place (upload, copy or RCCL broadcast): derived copies (fp16)
    int precision() const { return cfg_.precision; }
    // GM_TILE for the fp32-A row-epilogue GEMMs (embed, projection, FFN down, encoder_proj, decoder projection): by the planner's
    // occupancy rule on fp32 engines, never on fp16 engines (whose LAYER GEMMs take the fp16 tile path through lin16, always)
    int tile_ok() const { return cfg_.precision == 0 ? 1 : 0; }
    bool f16_tile() const { return f16_tile_; }
    const PackedLayout &layout() const { return L_; }

    int alloc_slot();                 // -1 when full; state zeroed (reference calloc, april_session.c:40-58)
    void free_slot(int slot);
    int live_slots() const { return live_.load(std::memory_order_relaxed); }      // (read by aas_create_session's least-loaded placement on any thread)

    // ---- batched hot path (one stepping thread).  A FLIGHT is everything enqueued between two host waits: frames are cut,
    // chunk steps (encoder + the three joiner/decision/decoder rounds, all on the device) and decoder refreshes are queued
    // back to back, and the host reads the 16-byte-per-round records once, at end_flight().
    // pcm arrives as `n_parts` windows that are gathered straight into pinned staging (total n_pcm samples)
    // `pass`: the resample / decode work and the frame observers of this call.  Returns the pinned block that receives the observers' records, laid
    // out by pass_layout.h (null: no descriptors of the four): its bytes are complete once the flight that was open during the call
    // has been waited for (close_flight() puts the copy in front of the flight's event), and the block is lent until
    // release_pass_block().  Stepping thread only.
    const uint8_t *fbank(int n_frames, const FbankFrameDesc *desc, const std::pair<const int16_t *, size_t> *parts, size_t n_parts, size_t n_pcm,
                         HostPool *pool = nullptr, const FrontPass &pass = FrontPass());
    // decode launches and the frames they decoded so far (any thread)
    void decode_counts(uint64_t *launches, uint64_t *frames) const
    {
        *launches = dc_launches_.load(std::memory_order_relaxed); *frames = dc_frames_.load(std::memory_order_relaxed);
    }
    // gives back the block a fbank() call lent; the scheduler calls it once per block, when it has read the pass's bytes.  Stepping thread only.
    void release_pass_block(const uint8_t *p);
    // ---- the frame observers (DESIGN.md sections 16, 17, 18, 21 and 22).  Launches of one observer's kernel and the frames they covered so far
    // (any thread; inline over plain members: the scheduler harness links session.cc against an engine of its own).  Nothing is allocated
    // for an observer until a pass carries one of its descriptors.
    void observer_counts(int id, uint64_t *launches, uint64_t *frames) const
    {
        *launches = obs_counts_[id].launches.load(std::memory_order_relaxed); *frames = obs_counts_[id].frames.load(std::memory_order_relaxed);
    }
    // aprilx_run_dtmf: n_runs runs in ONE launch; run r's n[r] frames (consecutive in `frames`, `padded` samples each) with plans[r].
    // powers_out (may be null): [sum n][9]
    void debug_dtmf(int n_runs, const DtmfPlan *plans, const int32_t *n, const int16_t *frames, uint8_t *codes_out, float *powers_out);
    // aprilx_run_dtmf_decide: the decision alone on n given rows of P[0..8), E
    void debug_dtmf_decide(const DtmfPlan &plan, int n, const float *powers9, uint8_t *codes_out);
    // aprilx_run_tones: n_runs runs in ONE launch, as debug_dtmf; records_out [sum n] (lo | hi << 16), powers_out (may be null) [sum n][F + 1]
    void debug_tones(int n_runs, const TonePlan *plans, const int32_t *n, const int16_t *frames, uint32_t *records_out, float *powers_out);
    // aprilx_run_quality: n_runs runs in ONE launch, as debug_dtmf, run r with clip level clip_levels[r] over hops of `hop` samples; records_out [sum n][8]
    void debug_quality(int hop, int n_runs, const int32_t *clip_levels, const int32_t *n, const int16_t *frames, uint32_t *records_out);
    // aprilx_run_tone_decide: the decision alone on n given rows of P[0..F), E
    void debug_tone_decide(const TonePlan &plan, int n, const float *powers, uint32_t *records_out);
    // aprilx_run_vad: n_runs runs in ONE launch over a scratch ring of ring_rows rows per run; run r's n[r] rows (consecutive in `rows`)
    // sit at rows (first_row[r] + i) % ring_rows of its ring
    void debug_vad(int n_runs, const VadPlan *plans, const int32_t *n, const int32_t *first_row, int ring_rows, const float *rows, VadState *states_io,
                   uint8_t *bytes_out, float *energy_out);
    void begin_flight();
    bool flight_has_room(int rows, int nsteps = 1) const;   // `nsteps` more steps with `rows` rows in total fit into the index / record rings
    // one chunk for m sessions (m <= max_batch): returns the step's index inside the flight.  logits_out (tests): when
    // non-null the step runs eagerly, waits, and returns the logits of the three rounds [3][m][vocab]
    int step(int m, const int *slots, const int *ring_tails, const int *now_ms, float *logits_out = nullptr);
    // Layer-major step: T consecutive chunks of each of m sessions (T * m <= max_batch rows) in one
    // go.  Everything that does not depend on the recurrence -- conv front end, the INPUT half of every layer's gate GEMM, the
    // feed-forward blocks, encoder_proj -- runs once over all T * m rows; only the recurrent half of the gates and the
    // projection run per time step.  Same chains, same order: logits and state are bit-identical to T one-chunk steps.
    // ring_tails / now_ms are [T][m].  Records: [T][3][m]; logits_out (tests) [T][3][m][vocab].
    // mode 1: the T chunk steps of one feed (T >= 2) as a wavefront over the layers -- the one-launch gates GEMM per chunk as in
    // step(), the same launch of the active layers z-batched (run_sw_chain); mode 0: layer-major (long feeds).
    int lm_step(int m, int T, const int *slots, const int *ring_tails, const int *now_ms, float *logits_out = nullptr, int mode = 0);
    int lm_max_rows() const { return cfg_.max_batch; }
    // decoder output refresh for listed slots from the context held on the device; op 1 = end-of-flush reset first
    void decode_rows(int n, const int *slots, int op);
    // end of a flight in two halves, so that the next flight can be enqueued before this one has run: close_flight() queues
    // the record copy and an event and returns the flight's parity (0 / 1); wait_flight(parity) blocks until the GPU has
    // passed that event, flight_done() polls it.  At most TWO flights are open at any time (begin_flight() reuses the parity
    // of the flight before the previous one: its records must have been read by then).
    int close_flight();
    bool flight_done(int parity);
    void wait_flight(int parity);
    void end_flight();                          // close + wait (records -> host)
    bool profiling() const { return profiling_; }
    // the scheduler's hint for the flight being launched: another flight is in the air (or follows at once), so a feed is worth
    // splitting over the three streams; a lone flight runs on one stream (the events between the streams cost it ~50 us)
    void set_overlap_hint(bool on) { overlap_hint_ = on; }
    const StepRecord *records(int step_index) const { return rec_h_ + rec_off_h_[step_index]; }   // [3][m], valid after end_flight()
    // ---- the per-slot opt-in tables: confidences, bias sets, search options (DESIGN.md sections 12-14).  ONE life cycle: set_slot_*()
    // only QUEUES the change (any thread, for an idle session's slot; inline over plain members: the scheduler harness links session.cc
    // against an engine of its own); an off value is dropped while nothing was ever on.  begin_flight() applies the queues on the stepping
    // thread (apply_slot_tables): the first opt-in of a table allocates it (device + pinned mirror; the captured pointer never changes
    // afterwards) and drops the captured graphs, whose decision launches were captured without it.
    // Confidences: K alternatives per slot (0 = off); the side ring is allocated with the table.
    void set_slot_confidence(int slot, int k) { conf_q_.push(slot, k, k > 0); }
    // side records of a step, indexed like records(); null while no session of the engine has opted in.  Valid after the
    // flight's wait for rows of opted-in sessions whose StepRecord is valid.
    const ConfRecord *conf_records(int step_index) const { return conf_h_ ? conf_h_ + rec_off_h_[step_index] : nullptr; }
    uint64_t confidence_records() const { return conf_copied_.load(std::memory_order_relaxed); }     // side records copied to the host so far
    // Phrase boosting: set_slot_bias() (null = off) also keeps the books -- which of the engine's kBiasSets table entries holds the set,
    // how many slots use it -- in the same critical section as the push; a set is uploaded the first time a slot of this engine uses it
    // and freed when no slot uses it any more (the descriptor table has a fixed capacity).  The slot's trie state returns to the root
    // with every change.  False: the table is full or the vocabulary is too large for the kernel.
    static constexpr int kBiasSets = 64;
    bool set_slot_bias(int slot, const std::shared_ptr<const BiasSet> &set)
    {
        std::lock_guard<std::mutex> g(bias_q_.mutex());
        if (slot < 0 || slot >= cfg_.max_slots) return false;
        if (bias_slot_set_.empty()) {
            if (!set) return true;                               // nothing was ever on
            bias_slot_set_.assign((size_t)cfg_.max_slots, -1); bias_sets_.resize(kBiasSets);
        }
        int idx = -1;
        if (set) {
            if (set->vocab != L_.dims.vocab || set->vocab > kBiasMaxVocab) return false;
            for (int i = 0; i < kBiasSets && idx < 0; ++i) if (bias_sets_[(size_t)i].set == set) idx = i;
            for (int i = 0; i < kBiasSets && idx < 0; ++i) if (!bias_sets_[(size_t)i].set) idx = i;
            // (an entry nobody uses any more becomes free when begin_flight has released its device copy)
            if (idx < 0) return false;
            bias_sets_[(size_t)idx].set = set;
            ++bias_sets_[(size_t)idx].users;
        }
        const int old = bias_slot_set_[(size_t)slot];
        if (old < 0 && idx < 0) return true;                     // no set before, none now (every aas_free comes through here): nothing to apply
        if (old >= 0) --bias_sets_[(size_t)old].users;
        bias_slot_set_[(size_t)slot] = idx;
        bias_q_.push_locked(slot, idx, idx >= 0);
        return true;
    }
    // the device's trie state of a slot; waits for the streams.  0 while no session of the engine has a set, and for a slot with a queued
    // change (begin_flight returns it to the root before the slot's next step)
    int read_bias_state(int slot);
    // Language models: the life cycle of the bias sets, with books of its own under lm_q_.mutex() -- a model is
    // shared by shared_ptr identity, uploaded the first time a slot of this engine uses it and freed when its last slot lets go; the
    // descriptor table holds kLmModels entries.  The slot's node returns to the model's start with every change.  False: all entries hold
    // other models, or the model was built for another vocabulary size.
    bool set_slot_lm(int slot, const std::shared_ptr<const LmSet> &set, float weight, float token_bonus)
    {
        std::lock_guard<std::mutex> g(lm_q_.mutex());
        if (slot < 0 || slot >= cfg_.max_slots) return false;
        if (lm_slot_model_.empty()) {
            if (!set) return true;                               // nothing was ever on
            lm_slot_model_.assign((size_t)cfg_.max_slots, -1); lm_models_.resize(kLmModels);
        }
        int idx = -1;
        if (set) {
            if (set->vocab != L_.dims.vocab || set->vocab > kLmMaxVocab) return false;
            for (int i = 0; i < kLmModels && idx < 0; ++i) if (lm_models_[(size_t)i].set == set) idx = i;
            for (int i = 0; i < kLmModels && idx < 0; ++i) if (!lm_models_[(size_t)i].set) idx = i;
            if (idx < 0) return false;
            lm_models_[(size_t)idx].set = set;
            ++lm_models_[(size_t)idx].users;
        }
        const int old = lm_slot_model_[(size_t)slot];
        if (old < 0 && idx < 0) return true;
        if (old >= 0) --lm_models_[(size_t)old].users;
        lm_slot_model_[(size_t)slot] = idx;
        lm_q_.push_locked(slot, LmSlot{idx, idx >= 0 ? weight : 0.0f, idx >= 0 ? token_bonus : 0.0f, set ? set->start : 0}, idx >= 0);
        return true;
    }
    // the device's node of a slot; waits for the streams.  For a slot with a queued change: the start node of the queued model (what
    // begin_flight writes before the slot's next step); 0 while no session of the engine has a model
    int read_lm_state(int slot);
    // decision launches of the LM forms issued so far (one captured into a graph counts once), models resident on the device now, uploads so far
    void lm_counts(uint64_t *launches, int32_t *resident, uint64_t *uploads) const
    {
        *launches = lm_launches_.load(std::memory_order_relaxed); *resident = lm_resident_.load(std::memory_order_relaxed); *uploads = lm_uploads_.load(std::memory_order_relaxed);
    }
    // Search options: endpoint_ms 0 = no options
    void set_slot_search_options(int slot, SearchOpt o) { opt_q_.push(slot, o, o.endpoint_ms != 0); }
    void sync();                               // stepping thread (or under capture_mu_): waits for the three streams and clears the cross-stream dependency flags
    void sync_streams();                       // any thread: waits for the three streams, nothing else

    // ---- debug / parity entry points (state passed explicitly, like the ORT tensors)
    void debug_encoder(int n, const float *x, const float *h, const float *c, float *eout, float *h2, float *c2);
    void debug_decoder(int n, const int64_t *ctx, float *dout);
    void debug_joiner(int n, const float *eout, const float *dout, float *logits);
    // parity tests of the device's copy of the search decision (aprilx_run_decide*, aprilx_run_confidence*): returns the records, the side
    // records and the new states
    void debug_decide(const DecideRequest &q);
    void debug_fbank(int n_frames, const int16_t *pcm_frames /*[n][padded]*/, float *out /*[n][nbins]*/);
    // one whole segment through resample_kernel (aprilx_resample); out holds resample_total(n) samples
    void debug_resample(const ResampleSpec *spec, const int16_t *pcm, size_t n, int16_t *out);
    // n_frames frames of `channels` interleaved values through decode_kernel (aprilx_decode); out holds n_frames samples
    void debug_decode(uint32_t encoding, uint32_t channels, int32_t channel, const void *data, size_t n_frames, int16_t *out);
    void read_ring(int slot, int row, int n_rows, float *out);
    void read_greedy_state(int slot, GreedyState *out);

    // ---- session snapshot / restore (engine.cc "snapshot").  A session's DEVICE BLOCK is the bytes of its slot's
    // rows of the arrays below, in this order, each at a 16-byte aligned offset; the ring contributes the rows the session's book can
    // still name.  The layout depends on the model's dimensions and the precision only.
    enum { SNAP_H = 0, SNAP_C = 1, SNAP_H16 = 2, SNAP_EOUT = 3, SNAP_DOUT = 4, SNAP_GSTATE = 5, SNAP_BIAS = 6, SNAP_VAD = 7, SNAP_RING = 8, SNAP_ARRAYS = 9 };
    struct SnapLayout {
        struct Arr { uint32_t layers = 0, row_bytes = 0, off = 0; } arr[SNAP_ARRAYS];      // (h16: 0 layers unless the engine keeps it; ring: layers 0, off = fixed)
        uint32_t fixed = 0;                                                                   // bytes in front of the ring rows
        uint32_t block_bytes(int ring_rows) const { return fixed + ((uint32_t)ring_rows * arr[SNAP_RING].row_bytes + 15u) / 16u * 16u; }
    };
    SnapLayout snapshot_layout() const;
    // Both: stepping thread only, between flights (Scheduler::run_on_loop).  ONE kernel launch and one staging copy for all n sessions;
    // they return after a stream wait.  recs[i]: slot, tail / tgt_tail, rows and mask from the caller (checked here: false, and nothing
    // is launched, on a slot, a row count or a tail out of range); block_bytes and stage_off are filled in.  Queued slot-table changes
    // are applied first (a restored trie state must not be returned to the root by a change that was still queued).
    bool snapshot_gather(int n, SnapRec *recs, uint8_t *const *blocks_out);
    bool snapshot_scatter(int n, SnapRec *recs, const uint8_t *const *blocks);
    // gather and scatter launches so far (any thread)
    void snapshot_counts(uint64_t *gathers, uint64_t *scatters) const
    {
        *gathers = snap_gathers_.load(std::memory_order_relaxed); *scatters = snap_scatters_.load(std::memory_order_relaxed);
    }

    // ---- profiling: when enabled every launch of the named classes is bracketed by hipEvents
    void set_profiling(bool on);
    // Gates clock (bench.py's roofline): while it is on, the feed-wavefront launch plans are built with a stamp slot per gates launch
    // (GemmArgs::stamp): the kernels time themselves under graph replay.  Switching it off reads the slots back.
    void set_gates_clock(bool on);
    void gates_clock(double *ms, long *launches, long *rows) const { *ms = gclk_ms_; *launches = gclk_launches_; *rows = gclk_rows_; }
    // ... and split by the number of problems sharing the launch (index min(n, 4) - 1): the three gates kernels of the trace
    // (one problem: gemm_f32_kernel, two: gemm_f32_zkernel, three at 256 sessions: gemm_f32_zkernel_walk) map onto it one to one
    void gates_clock_by_n(double *ms4, long *launches4) const { for (int i = 0; i < 4; ++i) { ms4[i] = gclk_ms_n_[i]; launches4[i] = gclk_launches_n_[i]; } }
    KernelTiming timing(int cls) const { return timing_[cls]; }
    // ramp merge: feeds whose head a predecessor's layer graph ran (the device's count, read back: exact once the streams are idle) and
    // split feeds launched as hostable (any thread)
    void ramp_counts(uint64_t *hosted, uint64_t *eligible);
    // ... and of the deferred enqueue (APRIL_RAMP_MERGE=1): headless layer graphs launched, deferrals settled by wait_flight / flight_done, by any other entry
    void ramp_defer_counts(uint64_t *headless, uint64_t *by_wait, uint64_t *by_other);
    void reset_timing();
    enum { T_GATES = 0, T_GEMM_OTHER = 1, T_ROW = 2, T_CONV = 3, T_FBANK = 4, T_DEC = 5, T_RESAMPLE = 6, T_DECODE = 7, T_VAD = 8, T_DTMF = 9, T_TONE = 10,
           T_SNAP_GATHER = 11, T_SNAP_SCATTER = 12, T_QUALITY = 13, T_COUNT = 14 };
    long kernels_per_step() const { return kernels_per_step_.load(std::memory_order_relaxed); }    // launches of the last eagerly issued chunk chain

private:
    void upload_tables(const FbankHostTables &ft);
    void zero_slots(int n);
    void run_encoder_rows(int n, const float *x_direct);
    void encoder_front(size_t r0, int rows, const int *row_slots, const float *x_direct, hipStream_t st, float *ws);
    void lm_stage_layer(int l, int m, int t0, int t1, hipStream_t st);
    void lm_stage_proj(int m, int t0, int t1, hipStream_t st, float *ws);
    // the encoder's GEMMs as argument blocks over rows [r0, r0 + rows) of the work buffers (engine.cc "encoder")
    enum { GATES_ALL = 0xF, GATES_X = 0x3, GATES_H = 0xC };      // forms of the gates GEMM = their wave masks
    RowScale in_scale(int l, size_t r0) const;
    GemmArgs args_gates(int l, size_t r0, int rows, int waves) const;
    GemmArgs args_whr(int l, size_t r0, int rows) const;
    GemmArgs args_ff1(int l, size_t r0, int rows) const;
    GemmArgs args_ff2(int l, size_t r0, int rows) const;
    GemmArgs args_encproj(size_t r0, int rows, const int *slot_idx, float *out) const;
    AdvanceArgs advance_args(int m, int T) const;
    // where one chunk's search reads its inputs and writes its records
    struct GreedyIo {
        int gen = 1;                          // generation of the chunk for the round flags / active marks (unique until they are cleared)
        const int *now = nullptr;             // [n] session times
        const float *eout = nullptr;          // null: the sessions' slot rows of eout_; else rows eout_rows[i] (or i) of this matrix
        const int *eout_rows = nullptr;
        const int *rec_off = nullptr; int rec_slot0 = 0;
        float *dump = nullptr;                // [3][n][vocab] or null
    };
    void run_greedy_rounds(int n, bool dump_logits, int chunk = 0, const float *eout_rows = nullptr);
    void run_greedy_rounds(int n, const GreedyIo &io);
    void run_lm_chain(int m, int T, bool dump_logits);
    void run_lm_wavefront(int m, int T, bool dump_logits);
    struct SwPlan {                          // argument blocks + launch list of run_sw_chain for one (m, T, parity); its captured graphs live in sw_graphs_
        struct Batch { size_t off; int n, macro, kind; size_t roff; int rn; };      // rn > 0: the GEMMs write partial planes, rn row problems finish them; kind 4: the ramp latch
        struct Chain { std::vector<GemmArgs> host; GemmArgs *dev = nullptr; std::vector<Batch> batches; std::vector<RowArgs> rhost; RowArgs *rdev = nullptr; };
        Chain one;                           // the one-stream graph and the eager path
        Chain split;                         // the layer graph of a split feed while the ramp merge is on (else empty: `one` serves it); guarded forms (APRIL_RAMP_MERGE=3 / 2): head steps behind head_live
        Chain headless;                      // APRIL_RAMP_MERGE=1: `split` from macro step RAMP_R + 1 on, for a feed whose head the chain in front of it ran
        bool hosts = false;                  // `split` and `headless` carry guest blocks and the latch in their last RAMP_R macro steps
        const Chain &layers(bool split_feed) const { return split_feed && !split.batches.empty() ? split : one; }
        std::vector<std::pair<int, long>> stamp_slots; std::vector<int> stamp_n;  // gates clock: (slot, rows) and problem count of every gates launch of a plan built while it was on
    };
    // keys of the current flight parity (it selects buffers); plans built under the gates clock carry stamp slots: -m; part 0: the one-stream graph, 1..3: a split feed's,
    // 4: its headless layer graph
    GraphCache::Key graph_key(int m, int T = 0, int part = 0) const { return {m, T, flight_parity_ * 8 + part}; }
    GraphCache::Key sw_key(int m, int T, int part = 0) const { return graph_key(gclk_ ? -m : m, T, part); }
    SwPlan &sw_plan(int m, int T);
    void build_sw_chain(SwPlan &p, SwPlan::Chain &c, int m, int T, bool ramp, bool headless = false);
    void free_sw_plans();                    // every plan's device blocks and graphs (streams drained, legacy lock held)
    void run_sw_chain(int m, int T, bool dump_logits, const SwPlan &p, int part, hipStream_t st);
    int stage_step(int m, int T, const int *slots, const int *ring_tails, const int *now_ms); void read_back_logits(int k, int rows, float *out);
    template <typename Chain> hipGraphExec_t cached_graph(GraphCache &cache, const GraphCache::Key &key, hipStream_t st, Chain &&chain);
    template <typename Capture> void capture_both_parities(Capture &&capture);
    void run_feed_wavefront(int m, int T, bool dump_logits); void run_layer_major(int m, int T, bool dump_logits); void launch_split_feed(int m, int T, hipStream_t fe);   // lm_step's paths
    struct StreamTrace { hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; int m = 0, T = 0; bool used = false, headless = false; };
    std::deque<StreamTrace> trace_; hipEvent_t trace_base_ = nullptr;
    StreamTrace *trace_slot();
    void dump_stream_trace();
    void select_parity(int p);
    void join(hipStream_t waiter, hipStream_t src);
    void general_prologue();
    int next_step_index() { ++flight_steps_; return (int)(step_seq_++ & (uint64_t)(2 * step_cap_ - 1)); }
    void launch_rowepi(GemmArgs fused_form, float *ws, hipStream_t st, bool force = false, int cls = T_GEMM_OTHER);
    bool gates_tile_rows(long rows) const;
    void run_decproj(int n, const int *d_slots, const int *row_mask, const int *run_flag, int run_gen, float *out = nullptr);
    void build_dec_table();
    void run_chain(int m, bool dump_logits);     // advance + encoder + greedy rounds with arguments that depend on m only
    void collect_gates_clock();                  // adds the stamp slots of every clocked plan to the sums
    void timed_begin(int cls);
    void timed_end(int cls);
    void collect_timing();
    DecEmbedParams dec_params() const;

    EngineConfig cfg_;
    PackedLayout L_;
    ModelParams P_;
    hipStream_t stream_ = nullptr;
    float *w_ = nullptr;                       // packed weights
    uint16_t *wh_ = nullptr;                   // fp16 copies of the GEMM weight sections (same offsets, in elements), precision 1 only
    void lin(GemmArgs &g, size_t off) const { if (wh_) { g.wp = wh_ + off; g.wt = 1; } else { g.wp = w_ + off; g.wt = 0; } }
    // fp16 tile path (BASELINE configs[4]; kernels_gemm_tile.hip WT = 1): the four GEMMs of a layer read binary16 activations
    // (written by the producing epilogues) and weights re-packed for v_mfma_f32_16x16x32_f16; every batch size takes it
    bool f16_tile_ = false;
    uint16_t *wx_ = nullptr;                   // x32-order binary16 copies of the layer GEMM weights (same offsets as w_)
    uint16_t *y16_ = nullptr, *xb16_ = nullptr, *u16_ = nullptr, *ff16_ = nullptr;   // [max_batch][d_model | d_model | hidden | ffn]
    uint16_t *h16_ = nullptr;                  // [L][slots][d_model] binary16 copy of h
    int kzx_hr_ = 1, kzx_ff2_ = 1;             // K slabs of the projection / FFN-down GEMMs on 32-k blocks
    void lin16(GemmArgs &g, size_t off) const { g.wp = wx_ + off; g.wt = 1; g.tile_ok = 2; }
    int kz_hr() const { return f16_tile_ ? kzx_hr_ : kz_hr_; }
    int kz_ff2() const { return f16_tile_ ? kzx_ff2_ : kz_ff2_; }
    float *h_ = nullptr, *c_ = nullptr, *ring_ = nullptr, *eout_ = nullptr, *dout_ = nullptr;
    GreedyState *gstate_ = nullptr;            // [slots]
    float *dec_table_ = nullptr;               // [vocab * vocab][joiner] decoder output of every context, or null (build_dec_table)
    uint8_t *cls_ = nullptr;                   // [vocab] token classes
    int ring_frames_ = 0;
    // work buffers
    float *xin_ = nullptr, *a3_ = nullptr, *y_ = nullptr, *ssq_ = nullptr, *xb_ = nullptr, *u_ = nullptr, *ff_ = nullptr, *ws_ = nullptr, *ws_g_ = nullptr, *de_ = nullptr;
    float *logits_ = nullptr;                  // [3][max_batch][vocab] (traced steps, debug_joiner)
    float *p_lm_ = nullptr, *eout_lm_ = nullptr;   // layer-major: input half of the gates [rows][4 hidden], encoder outputs [rows][joiner] (allocated on first use)
    // step bookkeeping: pinned host rings (read by the advance kernel) + device mirrors
    int *ring_h_ = nullptr; size_t ring_cap_ = 0, ring_pos_ = 0;      // index blocks (capacities are per flight parity)
    int *step_off_h_ = nullptr, *rec_off_h_ = nullptr; int step_cap_ = 0;
    StepRecord *rec_d_ = nullptr, *rec_h_ = nullptr; size_t rec_cap_ = 0, rec_pos_ = 0;
    int flight_parity_ = 0, next_parity_ = 0; size_t ring_base_ = 0, rec_base_ = 0; int flight_steps_ = 0;
    uint64_t step_seq_ = 0;                    // steps enqueued since the engine started = the device's step counter (advance_kernel)
    hipEvent_t flight_done_[2] = {nullptr, nullptr};
    // the per-slot opt-in tables: nothing below is allocated until a session opts in
    SlotQueue<int> conf_q_; DeviceTable<uint8_t> conf_k_;    // K per slot
    ConfRecord *conf_d_ = nullptr, *conf_h_ = nullptr;       // [2 * rec_cap_] side ring, indexed like rec_d_ / rec_h_ (allocated with conf_k_)
    std::vector<std::pair<size_t, size_t>> conf_spans_;      // (first record, count) of this flight's steps that hold an opted-in row
    std::atomic<uint64_t> conf_copied_{0};
    void apply_slot_tables();                  // begin_flight: the three queues -> the tables (engine.cc "slot tables")
    void drop_graphs();                        // (capture_mu_ held, streams drained) every captured graph; they are captured again at their next use
    struct BiasEntry { std::shared_ptr<const BiasSet> set; int users = 0; void *dev = nullptr; };      // dev: one allocation holding the four arrays
    SlotQueue<int> bias_q_; DeviceTable<int32_t> bias_set_;  // the table entry of every slot's set, or -1
    std::vector<BiasEntry> bias_sets_;                // [kBiasSets] (bias_q_.mutex())
    std::vector<int> bias_slot_set_;                  // [slots] the queued set of every slot (bias_q_.mutex())
    int32_t *bias_state_d_ = nullptr;                 // [slots] trie states
    DeviceTable<BiasDesc> bias_desc_;                 // [kBiasSets]
    SlotQueue<SearchOpt> opt_q_; DeviceTable<SearchOpt> opt_;
    BiasDesc upload_bias(const BiasSet &set, void **dev, hipStream_t st);
    struct LmEntry { std::shared_ptr<const LmSet> set; int users = 0; void *dev = nullptr; };           // dev: one allocation holding the eight arrays
    SlotQueue<LmSlot> lm_q_; DeviceTable<LmSlot> lm_slot_;    // the model, weight, bonus and start node of every slot (model -1 = none)
    std::vector<LmEntry> lm_models_;                  // [kLmModels] (lm_q_.mutex())
    std::vector<int> lm_slot_model_;                  // [slots] the queued model of every slot (lm_q_.mutex())
    int32_t *lm_state_d_ = nullptr;                   // [slots] node ids
    DeviceTable<LmDesc> lm_desc_;                     // [kLmModels]
    std::atomic<uint64_t> lm_launches_{0}, lm_uploads_{0};
    std::atomic<int32_t> lm_resident_{0};
    LmDesc upload_lm(const LmSet &set, void **dev, hipStream_t st);
    void note_conf_step(int k, const int *slots, int m, size_t records);
    bool flight_open_[2] = {false, false};     // flight_done_[p] has been recorded and not yet waited for by begin_flight (wait_flight leaves it set: waiting twice is free)
    // streams (engine.cc "streams"): front end / search beside the layer chain, the per-parity buffers that make it safe
    hipStream_t f_stream_ = nullptr, s_stream_ = nullptr, search_stream_ = nullptr;
    std::vector<hipEvent_t> join_ev_; size_t join_pos_ = 0;
    bool f_unseen_by_m_ = false, s_unseen_by_m_ = false, m_unseen_by_f_ = false, m_unseen_by_s_ = false, flight_tail_s_ = false;
    bool overlap_hint_ = false;
    int split_streams_ = 2;                    // APRIL_SPLIT_STREAMS: 0 = one stream, 1 = search on S, 2 = search on S + front end on F
    // ramp merge (engine.cc "ramp merge"): APRIL_RAMP_MERGE 0 = off, 1 = on with the deferred enqueue, 3 = on with the guarded head (the host does not look),
    // 2 = the guarded hosting plans and both kernels but never hostable
    int ramp_mode_ = 1;
    RampState *ramp_d_ = nullptr;            // the device words (kernels.h)
    // INVARIANT: m_quiet_ is true exactly while the layer graph of a split feed is the LAST thing enqueued on stream_ (M).  launch_split_feed sets it
    // behind that graph; every other enqueue on M -- general_prologue() and the direct users: slot zeroing, plan / option / bias / confidence uploads, a
    // profiled fbank, the debug entry points through sync() -- clears it BEFORE it enqueues.  Only then may the previous feed's window run this
    // feed's head: the guest problems overtake nothing that M was given in between.  (atomic: aas_free resets slots from client threads)
    // While a layer graph is deferred (below) it still holds -- the hosting chain IS the last thing on M --, and m_touched() settles the deferral first:
    // the deferred graph goes in front of whatever the caller is about to enqueue, as it would have without the deferral.
    std::atomic<bool> m_quiet_{false};
    void m_touched() { settle_pending_layers(true, RampDefer::BY_OTHER); m_quiet_.store(false, std::memory_order_release); }
    // Deferred enqueue (engine.cc "deferred enqueue"): a split feed offered to a chain with a latch has FE + ready kernel enqueued; its layer graph, search,
    // record copy and flight event follow when the latch's report of its generation is read.  defer_mu_ (a leaf: taken under capture_mu_ or alone, nothing
    // is locked under it) guards defer_, pend_ and the enqueue; defer_open_ mirrors defer_.pending() for the lock-free fast path.
    struct PendingFeed {
        int m = 0, T = 0, parity = 0; hipEvent_t fe_done = nullptr; StreamTrace *tr = nullptr; bool hosts = false;
        bool closed = false, pass_bytes = false; size_t rec_base = 0, rec_pos = 0; std::vector<std::pair<size_t, size_t>> conf_spans;      // close_flight() came while pending
    };
    RampDefer defer_; PendingFeed pend_; std::mutex defer_mu_; std::atomic<bool> defer_open_{false};
    unsigned long long *ramp_word_h_ = nullptr;      // the latch's report (pinned, coherent)
    uint32_t ramp_gen_h_ = 0;                        // ready kernels launched = the device's generation once they have run
    bool m_tail_latch_ = false;                      // the layer graph that m_quiet_ speaks of holds a latch (a hosting plan's)
    bool settle_pending_layers(bool wait, RampDefer::Who who);      // true: nothing is pending (any more)
    bool deferred_flight(int parity);
    void enqueue_split_layers(const PendingFeed &f, bool headless);
    void enqueue_flight_tail(hipStream_t tail, int parity, size_t rec_base, size_t rec_pos, const std::vector<std::pair<size_t, size_t>> &conf_spans);
    std::atomic<uint64_t> ramp_eligible_{0};
    float *xb_buf_[2] = {nullptr, nullptr}, *u_buf_[2] = {nullptr, nullptr}, *ff_buf_[2] = {nullptr, nullptr};      // per parity since guests of the other parity share a launch
    uint16_t *xb16_buf_[2] = {nullptr, nullptr}, *u16_buf_[2] = {nullptr, nullptr}, *ff16_buf_[2] = {nullptr, nullptr};
    float *y_buf_[2] = {nullptr, nullptr}, *ssq_buf_[2] = {nullptr, nullptr}, *eout_lm_buf_[2] = {nullptr, nullptr}, *ws_fe_ = nullptr, *ws_sr_ = nullptr;
    uint16_t *y16_buf_[2] = {nullptr, nullptr};
    int *step_buf_[2] = {nullptr, nullptr}, *flags_buf_[2] = {nullptr, nullptr}, *rec_off_buf_[2] = {nullptr, nullptr};
    int *counter_d_ = nullptr, *step_d_ = nullptr, *active_d_ = nullptr, *dirty_d_ = nullptr, *rec_off_d_ = nullptr, *flags_d_ = nullptr;
    int *dec_slots_d_ = nullptr;
    float *logits_h_ = nullptr;
    // fbank staging is double-buffered so the next call can fill one pair while the previous copy is in flight
    int16_t *hs_pcm_[2] = {nullptr, nullptr}, *ds_pcm_[2] = {nullptr, nullptr};      // one staging buffer per flip (staging_layout.h)
    StagingCaps fb_caps_;                      // what they have room for
    int fb_flip_ = 0;
    hipEvent_t fb_done_[2] = {nullptr, nullptr};
    std::vector<size_t> part_off_;             // staging offsets of the PCM windows of one fbank call
    std::atomic<uint64_t> dc_launches_{0}, dc_frames_{0};
    // voice activity: nothing below is allocated until a pass carries a VAD descriptor
    VadState *vad_state_d_ = nullptr;          // [slots] (a session's first descriptor carries VAD_RESET: never initialised by the host)
    uint8_t *pass_out_d_ = nullptr; size_t pass_out_cap_ = 0;      // one pass's block on the device (pass_layout.h; stream order keeps the passes apart)
    struct PassBlock { uint8_t *h = nullptr; size_t cap = 0; bool busy = false; };
    std::vector<PassBlock> pass_blocks_;         // pinned blocks, one per pass whose records (pass_layout.h) the scheduler has not read yet: lent by fbank(), busy until release_pass_block()
    bool pass_bytes_flight_ = false;                  // the open flight holds a pass with observers' records: its event must follow their copy on the front-end stream
    struct ObserverCount { std::atomic<uint64_t> launches{0}, frames{0}; } obs_counts_[OBS_COUNT];      // observer_counts()
    // DTMF: nothing below is allocated until a pass carries a DTMF descriptor
    const float *dt_tables_ = nullptr; int dt_wd_ = 0;      // [16][Wd] on the device, uploaded once (freed with table_allocs_)
    const float *dtmf_tables();
    // tones: nothing below is allocated until a pass carries a tone descriptor
    const float *tn_tables_ = nullptr; int tn_w_ = 0, tn_f_ = 0;      // [2F][W] on the device, uploaded once (freed with table_allocs_)
    const float *tone_tables();
    // (line quality: no table, no per-slot record)
    const float *upload_table(const std::vector<float> &t);      // a table to the device, kept until the engine goes (rs_mu_ held)
    // snapshot / restore: nothing below is allocated until the first call
    bool snapshot_copy(int n, SnapRec *recs, uint8_t *const *blocks, bool scatter);
    char *snap_d_ = nullptr, *snap_h_ = nullptr; size_t snap_cap_ = 0;      // device staging and its pinned twin: the records, then the blocks
    std::atomic<uint64_t> snap_gathers_{0}, snap_scatters_{0};
    std::mutex rs_mu_;
    std::map<const ResampleSpec *, const float *> rs_tables_;    // phase tables on the device, uploaded at first use (freed with table_allocs_)
    const float *resample_table(const ResampleSpec *spec);
    // fbank tables on device
    FbankTables ft_;
    std::vector<void *> table_allocs_;
    float pad_value_ = 0;
    // slots
    std::vector<int> free_, zero_pending_;     // free slots (reset), freed slots waiting for their reset launch
    void zero_pending_slots();
    std::atomic<int> live_{0};                  // written under slot_mu_, read without it (live_slots)
    std::mutex slot_mu_;
    std::mutex capture_mu_;                    // held while stream_ is being captured into a graph, and by other threads' enqueues
    // gemm split factors (fixed per shape => batch-invariant numerics)
    int kz_embed_ = 1, kz_hr_ = 1, kz_ff2_ = 1, kz_proj_ = 1, kz_out_ = 1;
    int ws_mstride_ = 0;
    float *conv_wt_ = nullptr;      // transposed weights of the first two convolutions: [9][ch0] then [ch0 * 9][ch1] (finish_weights)
    // captured launch chains: four families; APRIL_GRAPH_CACHE_CAP replaces all four capacities
    bool use_graphs_ = true;
    GraphCache step_graphs_{"chunk step", 256};          // {m, 0, parity}: second use, both parities
    GraphCache lm_graphs_{"layer-major chain", 32};      // {m, T, parity}: first use, this parity
    GraphCache lm_search_graphs_{"long-feed search", 64};  // {m, block length, parity}: first use, this parity
    GraphCache sw_graphs_{"feed wavefront", 5 * 64};     // sw_key(): second use, both parities; at most five graphs per plan, so sw_plans_ is full first: emptied with it
    size_t sw_plan_cap_ = 64;
    std::map<GraphCache::Key, SwPlan> sw_plans_;         // sw_key(m, T)
    // wavefront form of the layer-major step: its stream, events, per-launch argument blocks (pinned + device), the bookkeeping words of its search graphs
    hipStream_t lm_stream_ = nullptr;
    std::vector<hipEvent_t> lm_events_;
    GemmArgs *zargs_h_ = nullptr, *zargs_d_ = nullptr; size_t zargs_region_ = 0, zargs_pos_ = 0;     // three regions, round robin
    hipEvent_t zargs_done_[3] = {nullptr, nullptr, nullptr}; bool zargs_busy_[3] = {false, false, false}; int zargs_next_ = 0;
    int *lm_now_d_ = nullptr, *lm_rows_d_ = nullptr, *lm_rec_off_d_ = nullptr;
    std::atomic<long> kernels_per_step_{0};    // written by the stepping thread, read by aprilx_model_stats on any thread
    long launch_count_ = 0;
    // profiling
    bool profiling_ = false;
    bool gclk_ = false, gclk_warned_ = false; unsigned long long *gclk_slots_ = nullptr; int gclk_used_ = 0;      // gates clock (set_gates_clock): device slots of STAMP_WORDS (144) words
    static constexpr int GCLK_SLOTS = 2048;       // launch sites x 1152 B (STAMP_WORDS, kernels.h; layout: device_utils.h)
    double gclk_ms_ = 0; long gclk_launches_ = 0, gclk_rows_ = 0; double gclk_ms_n_[4] = {0, 0, 0, 0}; long gclk_launches_n_[4] = {0, 0, 0, 0};
    struct Ev { hipEvent_t a, b; int cls; };
    std::vector<Ev> ev_pool_; size_t ev_used_ = 0;
    KernelTiming timing_[T_COUNT];
};

}  // namespace aprilx
