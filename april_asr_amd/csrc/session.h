// Host-side session runtime for the GPU engine.
//
//   Greedy      the per-session transducer search + partial/final/silence state machine
//               (reference src/april_session.c:199-429), driven by the 16-byte per-round records
//               the device writes (arg-max, its logit, the blank logit) instead of 500-float logit
//               rows.  The decisions that steer the NEXT network call (blank or not, context push,
//               silence reset) are also taken on the device (kernels_misc.hip decide_kernel); the host
//               replays them from the same numbers when it builds the callbacks.
//   FrameBook   bookkeeping twin of the reference's OnlineFBank ring (src/fbank.c:98-127,
//               174-349): which frames exist, where they live in the HBM ring, flush padding.
//               The samples themselves only pass through (PCM16 FIFO -> pinned staging).
//   Scheduler   one stepping thread per GPU: gathers every session that has work, cuts new
//               frames (one fbank launch for all sessions), and advances all sessions with a
//               ready chunk in lock-step: one batched encoder pass, then three masked
//               joiner/decision/decoder rounds (reference src/april_session.c:431-476, batched),
//               chunk after chunk without waiting for the GPU; ONE wait per flight, then the
//               callbacks are replayed from the records.
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>
#include "../../include/april_api.h"
#include "../../include/aprilx_engine.h"
#include "bias.h"
#include "lm.h"
#include "engine.h"
#include "model_loader.h"

namespace aprilx {

enum TokClass : uint8_t {
    TK_WORD_START = 1,      // text[0] == ' '
    TK_SENT_END = 2,        // single char . ! ?
    TK_COMMA = 4,           // single char ,
    TK_DOT = 8,             // text[0] == '.'
    TK_DIGIT_START = 16     // text[0] in '0'..'9'
};
std::vector<uint8_t> classify_tokens(const ModelParams &p);

namespace snap { struct Access; }
struct JointResult { int32_t idx; float max_val; float blank_val; };     // what one joiner round hands to the search

struct Event {
    int type;                         // AprilResultType
    std::vector<AprilToken> tokens;
    // sessions with confidences on (aprilx_session_set_confidence): one entry per token, and tokens[i].reserved points to infos[i].
    // Events are only ever MOVED between containers (the vector's storage, and with it the pointers, stay where they are).
    std::vector<AprilxTokenInfo> infos;
    // a detector's event: type = kVadEventBase + kind, kDtmfEventBase + kind (section 17) or kToneEventBase + kind
    // (section 18) at time_ms; `digit` is a DTMF event's key, f1 and f2 a tone event's frequencies
    uint64_t time_ms = 0;
    char digit = 0;
    uint32_t f1 = 0, f2 = 0;
    // a line-quality event (section 21): type = kQualityEventBase + kind, and the event as its handler receives it
    std::unique_ptr<QualityEvent> quality;
};
constexpr int kVadEventBase = 0x100, kDtmfEventBase = 0x200, kToneEventBase = 0x300, kQualityEventBase = 0x400;
// where a session's events go: token events to `result`, voice-activity events to `vad`, DTMF events to `dtmf`, tone events to `tone`
// (null: dropped)
struct Handlers {
    AprilRecognitionResultHandler result = nullptr; void *userdata = nullptr;
    AprilxVadHandler vad = nullptr; void *vad_userdata = nullptr;
    AprilxDtmfHandler dtmf = nullptr; void *dtmf_userdata = nullptr;
    AprilxToneHandler tone = nullptr; void *tone_userdata = nullptr;
    AprilxQualityHandler quality = nullptr; void *quality_userdata = nullptr;
};
// the handler once per event, in order (null token pointer when an event has no tokens); `ev` is empty afterwards
void deliver_events(std::vector<Event> &ev, const Handlers &to);

class Greedy {
public:
    static constexpr int kMaxActive = 72;     // reference src/april_session.h:30
    void init(const ModelParams *p, const std::vector<uint8_t> *cls);
    // consume one joiner result; returns true when the round resolved to blank (chunk done)
    bool on_joint(const JointResult &r, float early_emit, size_t now_ms, std::vector<Event> &out);
    // end of flush: FINAL, clear context, SILENCE (reference src/april_session.c:561-563)
    void finish_flush(std::vector<Event> &out);
    void reset_context_to_blank();            // first use: context = [blank, blank]
    // confidences: K alternatives per delivered token, 0 = off.  With K > 0 the caller hands the round's
    // side record to set_side() before each on_joint(); the token's AprilxTokenInfo is kept beside active_[] and travels with it.
    void set_confidence(int k) { conf_k_ = k; }
    int confidence() const { return conf_k_; }
    void set_side(const ConfRecord *side) { side_ = side; }
    // phrase boosting: the session's bias set and the host's own copy of the trie state, advanced where the
    // context is pushed / cleared.  The replay does not need it (the records carry the biased arg-max); it is the independent
    // derivation the device's state is checked against (aprilx_session_bias_state).
    void set_bias(std::shared_ptr<const BiasSet> set) { bias_ = std::move(set); bias_state_ = 0; }
    const BiasSet *bias() const { return bias_.get(); }
    int bias_state() const { return bias_state_; }
    // language model: the session's model and the host's own copy of its node, advanced wherever the bias state is
    // advanced or cleared.  The replay does not need the model (the records carry the fused arg-max); the copy is the independent derivation
    // the device's node is checked against (aprilx_session_lm_state).
    void set_lm(std::shared_ptr<const LmSet> lm, float weight, float token_bonus)
    {
        lm_ = std::move(lm); lm_state_ = lm_ ? lm_->start : 0; lm_weight_ = lm_ ? weight : 0.0f; lm_bonus_ = lm_ ? token_bonus : 0.0f;
    }
    const LmSet *lm() const { return lm_.get(); }
    int lm_state() const { return lm_state_; }
    float lm_weight() const { return lm_weight_; }
    float lm_token_bonus() const { return lm_bonus_; }
    // search options: null = none (the lines below run as they always did); else the endpoint silence E replaces
    // the 2200 ms, bl' = bl - p replaces the blank logit in the three comparisons, and U > 0 caps the utterance length at a word boundary
    void set_search_options(const AprilxSearchOptions *o)
    {
        has_opt_ = o != nullptr;
        endpoint_ms_ = o ? o->endpoint_silence_ms : 2200; max_utt_ms_ = o ? o->max_utterance_ms : 0; blank_penalty_ = o ? o->blank_penalty : 0.0f;
    }
    bool has_search_options() const { return has_opt_; }
    AprilxSearchOptions search_options() const { return AprilxSearchOptions{(uint32_t)sizeof(AprilxSearchOptions), endpoint_ms_, max_utt_ms_, blank_penalty_}; }
    int ctx[2] = {0, 0};
    bool ctx_dirty = false;                   // decoder must be re-run for this session

private:
    friend struct snap::Access;               // snapshot.h: the state below as an image and back
    void push_ctx(int tok);
    void clear_context();
    void finalize_all(std::vector<Event> &out);
    void finalize_before_word(const AprilToken &incoming, std::vector<Event> &out);
    void emit_silence(std::vector<Event> &out);
    bool emit_partial(const AprilToken *tok, int tok_id, bool force, std::vector<Event> &out);
    void call(int type, size_t count, std::vector<Event> &out);

    const ModelParams *P_ = nullptr;
    const std::vector<uint8_t> *cls_ = nullptr;
    AprilToken active_[kMaxActive];
    int active_id_[kMaxActive];
    AprilxTokenInfo info_[kMaxActive];        // (conf_k_ > 0) beside active_[]: moved and dropped with it
    AprilxTokenInfo cur_info_;                // the info of the round on_joint is working on
    void fill_info(uint64_t eval_index);
    int conf_k_ = 0;
    const ConfRecord *side_ = nullptr;
    std::shared_ptr<const BiasSet> bias_;
    int bias_state_ = 0;
    std::shared_ptr<const LmSet> lm_;
    int lm_state_ = 0;
    float lm_weight_ = 0.0f, lm_bonus_ = 0.0f;
    uint64_t evals_ = 0;                      // joiner evaluations consumed so far = rows aprilx_session_trace_logits has written
    size_t head_ = 0, last_call_head_ = 0;
    bool emitted_silence_ = true;
    size_t last_emit_ms_ = 0;
    bool has_opt_ = false;
    uint32_t endpoint_ms_ = 2200, max_utt_ms_ = 0;
    float blank_penalty_ = 0.0f;
    size_t first_ms_ = 0;                     // time_ms of the first token put into active_[] since it was last emptied (head_ > 0)
};

struct FrameBook {
    int shift = 0, padded = 0, seg_count = 0, seg_step = 0, ring_frames = 0;
    int head = 0, tail = 0;
    long avail = 0, avail_shadow = 0;
    uint64_t rows_written = 0;      // ring rows written since the session started (real frames + flush padding)
    std::vector<int16_t> fifo;      // samples not yet fully consumed by framing
    size_t fifo_pos = 0;            // start of the next frame inside the stream  fifo ++ ext  (may point into ext)
    // A caller that blocks until its feed is processed LENDS its buffer: the samples are staged for the GPU straight from
    // there (one copy: caller -> pinned staging); only the unconsumed tail (less than a frame, normally) moves into the
    // fifo when the tick ends (settle()).
    const int16_t *ext = nullptr; size_t ext_cnt = 0;
    // Resampled input (aprilx_session_set_input_rate; `rs` non-null): fifo ++ ext then hold INPUT-rate samples, while every
    // position above (fifo_pos, stream_end(), the frames) stays a model-rate position -- absolute, counted from the session's
    // first sample.  The model-rate stream is the segments' outputs in order: segment s covers positions [pos, next segment's pos),
    // its output j at pos + j; outputs past the segment's end (the flush zeros behind it) are 0.  Input samples are numbered
    // across segments: fifo[0] is input `in_drop`, segment s starts at input in_start.
    struct RsSeg { int64_t pos = 0, in_start = 0, n_in = 0, n_out = 0, zeros = 0; bool closed = false; };
    const ResampleSpec *rs = nullptr;
    std::deque<RsSeg> segs;                     // segments whose outputs frames may still need; the last one is the current one
    int64_t in_drop = 0;
    int64_t rs_end = 0;                         // model-rate stream end (available outputs + flush zeros)
    // Input format (aprilx_session_set_input_format; `fmt` set): the queued and unconsumed audio is `raw` -- bytes, one
    // frame per position -- in place of fifo ++ ext, and the positions are kept by the segments above as for resampled input: with an
    // input rate the raw frames are the resampler's input samples, without one they are the stream's samples themselves (the identity
    // conversion L = M = 1, K = 0, which runs no resampler).  Flush zeros are int16 zeros behind a segment either way, never encoded.
    InputFormat fmt;
    RawFifo raw;
    bool segmented() const { return rs || fmt; }
    size_t held() const { return fmt ? raw.count() : fifo.size() + ext_cnt; }      // positions held in fifo ++ ext
    bool lent() const { return fmt ? raw.ext != nullptr : ext != nullptr; }
    size_t stream_end() const { return segmented() ? (size_t)rs_end : fifo.size() + ext_cnt; }
    void rs_update();                           // after samples were appended: the current segment's input count and available outputs
    void rs_close();                            // flush: the current segment is complete, all its outputs become available
    void rs_zeros(int64_t n);                   // flush zeros behind the closed segment
    int64_t rs_keep() const;                    // first input sample (numbered across segments) that frames may still need
    void set_rate(const ResampleSpec *spec) { set_input(spec, fmt); }      // idle session after creation / a completed flush
    void set_input(const ResampleSpec *spec, const InputFormat &f);         // the same for rate and format together
    bool chunk_ready() const { return avail >= seg_count; }
    bool can_cut() const { return stream_end() - fifo_pos >= (size_t)padded && avail + 1 <= ring_frames; }
    void absorb_ext();              // ext -> fifo (keeps stream positions valid)
    void settle();                  // end of tick: drop consumed samples, keep the tail, forget the lent buffer
    typedef std::vector<std::pair<const int16_t *, size_t>> Parts;
    void append_span(size_t l0, size_t l1, Parts &parts) const;     // samples [l0, l1) of fifo ++ ext (l0 < l1) as at most two parts
    FbankFrameDesc write_row(int slot, int pcm_off);     // one more ring row (pcm_off -1: flush padding); a real frame's caller moves avail_shadow and fifo_pos
    bool flush_allowed() const { return avail_shadow >= -(long)(seg_count * 3); }
    void compact();
};

class Scheduler;
struct Model;

struct Session {
    Model *model = nullptr;
    Scheduler *sched = nullptr;
    Engine *eng = nullptr;
    int slot = -1;
    Handlers handlers;                        // (the detectors' handlers change with their options, below)
    bool sync_mode = true, realtime_flag = false;

    // ---- guarded by Scheduler::mu_
    std::vector<int16_t> inbox;               // queued PCM (appended by callers; capacity is reused across feeds)
    // a session with an input format: frame_bytes > 0, its queue is raw_inbox (whole frames) and borrow_ptr / borrow_cnt lend raw FRAMES
    size_t frame_bytes = 0;
    std::vector<uint8_t> raw_inbox;
    size_t queued() const { return frame_bytes ? raw_inbox.size() / frame_bytes : inbox.size(); }      // positions in the inbox
    const short *borrow_ptr = nullptr;        // PCM lent by a caller that blocks until the work is done (sync feed, feed_many):
    size_t borrow_cnt = 0;                    //   copied once, by the stepping thread, outside the lock
    bool fed = false;                         // a feed arrived since the last collection (even an empty one)
    bool flush_requested = false;
    bool busy = false;                        // owned by the stepping thread right now (inflight > 0)
    int inflight = 0;                         // ticks of this session that have been collected and not completed yet (<= 2)
    bool closing = false;
    uint64_t submitted = 0, completed = 0;    // work tickets
    std::chrono::steady_clock::time_point oldest_submit;   // when the oldest work not yet collected by the stepping thread was handed over
    bool has_oldest = false;
    std::vector<Event> done_events;           // sync sessions: events waiting for the caller thread
    std::atomic<bool> delivering{false};      // a caller thread is inside deliver_sync_events() for this session ...
    std::thread::id delivering_tid;           // ... this one (written before `delivering` is set)
    // (both read under Scheduler::mu_) everything queued so far has been processed ...
    bool idle() const { return closing || (completed >= submitted && !busy && !fed && !flush_requested); }
    // ... and nothing is queued, no segment is open, no flush is under way: the session's options may change
    bool settable() const { return !(closing || busy || fed || flush_requested || !inbox.empty() || !raw_inbox.empty() || borrow_cnt || seg_open || flush_phase); }

    // ---- owned by the stepping thread while busy
    FrameBook fb;
    Greedy greedy;
    bool dout_ready = false;
    bool compact_pending = false;
    struct Replay { int step; int row; int rows; uint32_t now_ms; int kind; int chunk; };   // kind 0: chunk `chunk` of step (3 rounds of records), 1: end of flush
    std::vector<Replay> replay;               // what the open flights did for this session, in order (a flight consumes its own items from the front)
    std::atomic<double> speed_needed{1.0};    // reference src/april_session.c:79,456-462 (EMA of processing time / audio time x 1.1);
                                              // written by the stepping thread, read by aas_realtime_get_speedup from any thread
    bool was_flushed = false;
    bool seg_open = false;                    // audio was fed since creation or since the last flush (aprilx_session_set_input_rate refuses then)
    size_t ring_limit = 48000;                // asynchronous sessions: CANT_KEEP_UP bound (reference src/audio_provider.c:31, 3 s at the input rate)
    int flush_phase = 0;                      // 0 none, 1 pad-drain, 2 zeros, 3 pad-drain, 4 finish
    size_t now_ms = 0;
    uint64_t chunks = 0;
    std::vector<Event> events;                // produced during the current tick
    // The detectors (DESIGN.md sections 16, 17 and 18).  Options, plan and handler (in `handlers`) change only while the session is settable; the
    // rest is the stepping thread's while the session is busy.  real_frames: every real frame cut since creation, the frame clock of all.
    uint64_t real_frames = 0;
    struct Vad {
        bool on = false; VadOptions opt; VadPlan plan;
        bool reset = true;                    // the session's next descriptor starts from the reset state (the device keeps the detector's state)
        uint64_t speech = 0; uint32_t segments = 0; int last = 0;      // since the detector was last set: frames with the speech bit, SPEECH_START events; bit 0 of the last byte read
    } vad;
    struct Dtmf {
        bool on = false; DtmfOptions opt; DtmfPlan plan;
        DtmfMachine m;                        // (the device keeps nothing)
        uint64_t tone = 0, digits = 0;        // frames with a non-zero code, DOWN events, since the detector was last set
    } dtmf;
    struct Tones {
        bool on = false; ToneOptions opt; TonePlan plan;
        ToneMachine m;                        // (the device keeps nothing)
        uint64_t tonal = 0, tones = 0;        // frames with a tonal record, ON events, since the detector was last set
    } tones;
    struct Quality {                          // 
        bool on = false; QualityOptions opt; QualityPlan plan;
        QualityMachine m;                     // (the device keeps nothing)
        uint64_t frames = 0, clipped = 0, dead = 0, clip_samples = 0, reports = 0;      // records read, clipped and dead frames, clipped samples, REPORT events, since the observer was last set
    } quality;
    bool observes(int o) const { const bool on[OBS_COUNT] = {vad.on, dtmf.on, tones.on, quality.on}; return on[o]; }      // (by Observer)
    // tracing (tests): every joiner call appends `vocab` floats
    float *trace_buf = nullptr; size_t trace_cap = 0; size_t *trace_used = nullptr;
};

struct SchedStats {
    uint64_t ticks = 0, steps = 0, chunks = 0, rounds = 0, frames = 0, max_batch_seen = 0, flights = 0, replay_mismatch = 0, lm_steps = 0, lm_chunks = 0, wave_steps = 0, wave_chunks = 0;
    // host wall time of the stepping thread by phase (ms): 0 collect, 1 cut frames (host), 2 fbank call, 3 step enqueue,
    // 4 end of flight (wait for the GPU), 5 replay (decisions + events), 6 decoder refresh enqueue, 7 deliver/complete
    double host_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    void add(const SchedStats &o) {
        ticks += o.ticks; steps += o.steps; chunks += o.chunks; rounds += o.rounds; frames += o.frames; flights += o.flights; replay_mismatch += o.replay_mismatch;
        lm_steps += o.lm_steps; lm_chunks += o.lm_chunks; wave_steps += o.wave_steps; wave_chunks += o.wave_chunks;
        if (o.max_batch_seen > max_batch_seen) max_batch_seen = o.max_batch_seen;
        for (int i = 0; i < 8; ++i) host_ms[i] += o.host_ms[i];
    }
};

class Scheduler {
public:
    Scheduler(Model *m, Engine *e);
    ~Scheduler();
    void attach(Session *s);
    bool detach(Session *s);                       // waits until the session is idle; false = refused (called from the session's own handler)
    // queue work for n sessions at once and (for sync sessions / wait=true) block until it is done
    // `borrow`: the caller keeps the PCM buffers alive and unchanged until the sessions are idle again (it blocks in this
    // call, or drains afterwards), so they are read in place by the stepping thread instead of being copied under the lock
    // `bytes`: counts are bytes (aprilx_session_feed_bytes); else shorts, which a session with a format reads as 2 x count bytes.  A count
    // that is not a whole number of the session's frames: with `bytes`, false and nothing is queued for any session; else that session's
    // feed is dropped with an error message
    bool submit(int n, Session *const *ss, const short *const *pcm, const size_t *counts, bool flush, bool wait, bool borrow = false, bool bytes = false);
    void deliver_sync_events(Session *s);          // caller-thread delivery for sync sessions
    void wait_idle(Session *s);                    // everything queued so far has been processed
    // aprilx_session_set_input_rate: false when audio is queued or the session has an open segment
    bool set_input_rate(Session *s, const ResampleSpec *spec);
    // aprilx_session_set_input_format: the same rule; frame_bytes 0 = back to mono PCM16
    bool set_input_format(Session *s, const InputFormat &f);
    // aprilx_session_set_confidence: the same rule
    bool set_confidence(Session *s, int k);
    // aprilx_session_set_bias: the same rule; null = off.  False also when the engine has no room for another set
    bool set_bias(Session *s, std::shared_ptr<const BiasSet> set);
    bool set_lm(Session *s, std::shared_ptr<const LmSet> lm, float weight, float token_bonus);
    // aprilx_session_set_search_options: the same rule; null = back to no options
    bool set_search_options(Session *s, const AprilxSearchOptions *o);
    // aprilx_session_set_vad / _dtmf / _tones / _quality: the same rule; plan null = off.  The observer's state (VAD: on the device, from the
    // session's next descriptor on; the others: the machine) and its counters start afresh
    bool set_vad(Session *s, const VadOptions *o, const VadPlan *plan, AprilxVadHandler handler, void *userdata);
    bool set_dtmf(Session *s, const DtmfOptions *o, const DtmfPlan *plan, AprilxDtmfHandler handler, void *userdata);
    bool set_tones(Session *s, const ToneOptions *o, const TonePlan *plan, AprilxToneHandler handler, void *userdata);
    bool set_quality(Session *s, const QualityOptions *o, const QualityPlan *plan, AprilxQualityHandler handler, void *userdata);
    void wait_idle_many(Session *const *ss, int n);
    // until every listed session has at most `max_open` feeds that were submitted and not completed yet (pipelined group feeds)
    void wait_backlog(Session *const *ss, int n, uint64_t max_open);
    SchedStats stats();
    // hand-over -> delivery latencies (ms) of the last completed ticks, oldest first: from the submit() that queued the oldest work a
    // flight served to the moment its results were delivered (asynchronous handlers have run; synchronous callers have been released)
    size_t latencies(double *out, size_t cap, bool reset);
    Engine *engine() { return eng_; }
    bool on_loop_thread() const { return std::this_thread::get_id() == loop_tid_; }
    // Runs `fn` on the stepping thread BETWEEN flights -- every flight that was launched has completed, none is launched until fn returns --
    // and waits for it.  Work that must not meet a graph capture or a flight in the air (snapshot / restore) goes
    // through here.  fn runs without mu_.  False, and fn does not run: called from the stepping thread itself (a handler), or the
    // scheduler is stopping.
    bool run_on_loop(const std::function<void()> &fn);
    // the calling thread is inside one of this session's handlers right now (asynchronous: the stepping thread; synchronous: its caller's)
    bool in_own_handler(const Session *s) const { return on_loop_thread() || (s->delivering.load(std::memory_order_acquire) && s->delivering_tid == std::this_thread::get_id()); }

private:
    // one launched flight: the sessions it serves, their tickets, and how many replay items / chunks it added per session
    struct Flight {
        int parity = -1;                                     // the engine's flight id (Engine::close_flight)
        bool final = true;                                   // false: the rings filled up, the same tick continues in the next flight
        std::vector<Session *> work;
        std::vector<uint64_t> taken;
        std::vector<uint32_t> mark;
        std::vector<uint64_t> chunks0, chunks1;
        std::chrono::steady_clock::time_point t0;
        std::chrono::steady_clock::time_point t_sub;          // hand-over of the oldest work in the flight (submit() of any of its sessions)
        bool has_sub = false;
        uint64_t seq = 0;                                    // launch order: the pass records cut under this flight carry it
    };
    void loop();
    bool collect(std::vector<Session *> &work, std::vector<uint64_t> &taken, bool block, uint64_t &work_seen);
    Flight launch_flight(const std::vector<Session *> &work, const std::vector<uint64_t> &taken);
    void complete_flight(Flight &f);
    void cut_frames(std::vector<Session *> &work, bool &progressed);
    void stage_resampled(const FrameBook &fb, int64_t first, int64_t last_end, size_t base, size_t &staged_in);
    void stage_decoded(const FrameBook &fb, int64_t first, int64_t last_end, size_t base);
    void stage_raw(const FrameBook &fb, size_t l0, int32_t n_src, int32_t out_cnt, int32_t dst, bool dst_in);
    bool step_chunks(std::vector<Session *> &ready);     // false: the flight's rings are full, (some) work is left for the next flight
    // how advance() runs its T chunks: one chunk step (T == 1, Engine::step), or Engine::lm_step as a feed wavefront / layer-major
    enum StepPath { STEP_CHUNK, STEP_WAVE, STEP_LAYER_MAJOR };
    bool advance(Session *const *group, int m, int T, StepPath path);
    template <class Apply> bool configure(Session *s, Apply apply);     // the set_* calls: wait_idle, lock, refuse unless settable, apply
    // the four observers' set_* calls: the session's member `obs` afresh (on, with options and plan, or off) and its two handler slots
    template <class Obs, class Opt, class Plan, class Handler>
    bool set_observer(Session *s, Obs Session::*obs, Handler Handlers::*slot, void *Handlers::*slot_userdata, const Opt *o, const Plan *plan, Handler handler, void *userdata);
    void replay(Flight &f);
    // The pass queue: what the observers' kernels wrote for the passes of the open flights ("the pass's bytes").
    // cut_frames() pushes one record per pass that has runs, under the flight that is open; harvest(), once that flight has been waited
    // for, turns the runs into events, gives the block back to the engine and pops the record.  The record is the block's one owner.
    struct PassRun { Session *s; uint64_t t0; int32_t n, off; };      // frames [t0, t0 + n) at record `off` of its observer's part; n < 0: a flush completed at frame t0
    // block: Engine::fbank()'s, laid out by `at` (null: a pass of flush markers only); runs: by Observer
    struct PassPending { uint64_t flight = 0; const uint8_t *block = nullptr; PassLayout at; std::vector<PassRun> runs[OBS_COUNT]; };
    std::deque<PassPending> pass_pending_;
    std::vector<VadDesc> vdesc_; std::vector<DtmfDesc> tdesc_; std::vector<ToneDesc> ndesc_; std::vector<QualityDesc> qdesc_;       // scratch of cut_frames()
    uint64_t flight_seq_ = 0;
    const int shift_ms_;
    // records == null: the run is a flush marker; else the run's r.n records in the pass's block
    void harvest(uint64_t flight);
    void harvest_vad(const PassRun &r, const uint8_t *records);
    void harvest_dtmf(const PassRun &r, const uint8_t *records);
    void harvest_tone(const PassRun &r, const uint32_t *records);
    void harvest_quality(const PassRun &r, const uint32_t *records);
    int split_sticky_ = 0;
    int pipeline_depth_ = 2;                             // APRIL_PIPELINE: 2 = launch the next flight before completing the current one, 1 = one flight at a time

    Engine *eng_;
    const int stride_ms_;                          // audio time of one chunk step (segment_step frames)
    HostPool pool_;                                // helpers for the per-session host copies (APRIL_HOST_THREADS, default 3)
    std::mutex mu_;
    std::condition_variable cv_work_, cv_done_;
    // spin-then-block on both sides of the hand-over (a condition-variable wake-up costs 30..60 us each way, which is 5 %
    // of a 2 ms step): submit() bumps work_seq_, the end of a tick bumps done_seq_
    std::atomic<uint64_t> work_seq_{0}, done_seq_{0};
    int spin_step_us_ = 1000, spin_wait_us_ = 3000;   // APRIL_SPIN_STEP_US / APRIL_SPIN_WAIT_US
    std::chrono::steady_clock::time_point prev_done_;   // when the previous flight completed (stepping thread only): start of the next flight's own span
    bool have_prev_done_ = false;
    int wave_min_chunks_ = 2;                        // APRIL_WAVE_MIN_CHUNKS (0 = chunk steps one by one): chunk steps of one feed as a wavefront ...
    static constexpr int wave_max_chunks_ = 7;       // ... of at most this many chunks
    int lm_min_chunks_ = 8;                          // APRIL_LM_MIN_CHUNKS: sessions with at least this many chunks waiting take the layer-major path (0 = never)
    std::vector<Session *> sessions_;
    struct LoopCall { const std::function<void()> *fn; bool done = false; };
    std::vector<LoopCall *> calls_;                // guarded by mu_: run_on_loop() requests the stepping thread has not served yet
    std::atomic<int> calls_waiting_{0};
    bool stop_ = false;
    std::thread thread_;
    SchedStats stats_;                             // guarded by mu_
    SchedStats tick_;                              // the stepping thread's own; merged into stats_ under mu_ at the end of a tick
    std::vector<float> lat_ms_;                    // guarded by mu_: ring of the last kLatRing hand-over -> delivery latencies
    uint64_t lat_n_ = 0;
    static constexpr size_t kLatRing = 8192;
    std::chrono::steady_clock::time_point collect_t_sub_; bool collect_has_sub_ = false;   // stepping thread: oldest hand-over among the work of the last collect()
    std::thread::id loop_tid_;
    // scratch reused across ticks
    std::vector<FbankFrameDesc> desc_;
    FrameBook::Parts pcm_parts_;                   // windows to stage, in order
    FrameBook::Parts in_parts_;                    // input-rate spans of resampled sessions' windows, in order
    std::vector<ResampleDesc> rdesc_;
    std::vector<const ResampleSpec *> rspec_;
    std::vector<DecodeDesc> ddesc_;                // decode work of formatted sessions' windows
    RawFifo::Parts raw_parts_;                     // their raw bytes, in order (null parts: the padding in front of a span)
    size_t staged_raw_ = 0;                        // bytes of raw_parts_
    std::vector<int> slots_, tails_, now_;
    std::vector<float> logit_stage_;
};

struct LoadInfo { double broadcast_ms = 0, comm_init_ms = 0; size_t broadcast_bytes = 0; int ranks = 1, used_rccl = 0; };

struct Model {
    LoadInfo load;                            // how the weights reached the engines
    HostModel host;                           // params, tokens, names (weights freed after upload)
    PackedLayout layout;
    FbankHostTables ftab;
    std::vector<uint8_t> tok_class;
    std::map<uint32_t, ResampleSpec> resamplers;   // per input rate, built at first use (guarded by mu); never freed before the model
    std::vector<Engine *> engines;
    std::vector<Scheduler *> scheds;
    std::vector<float> host_blob;             // only for host-only models (no engine): packed weights
    std::mutex mu;
    ~Model();
};

}  // namespace aprilx
