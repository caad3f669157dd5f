// See session.h.
#include "session.h"
#include <algorithm>
#include <cstring>
#include "common.h"
#include "env.h"

namespace aprilx {

namespace {
struct Lap {
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    double operator()() { auto n = std::chrono::steady_clock::now(); double ms = std::chrono::duration<double, std::milli>(n - t).count(); t = n; return ms; }
};
}  // namespace

// ---------------------------------------------------------------- token classes
std::vector<uint8_t> classify_tokens(const ModelParams &p)
{
    std::vector<uint8_t> c((size_t)p.token_count, 0);
    for (int i = 0; i < p.token_count; ++i) {
        const char *t = p.token((size_t)i);
        uint8_t f = 0;
        if (t[0] == ' ') f |= TK_WORD_START;                                   // april_session.c:338
        const bool single = t[0] != 0 && t[1] == 0;
        if (single && (t[0] == '.' || t[0] == '!' || t[0] == '?')) f |= TK_SENT_END;   // :341
        if (single && t[0] == ',') f |= TK_COMMA;                              // :342
        if (t[0] == '.') f |= TK_DOT;
        if (t[0] >= '0' && t[0] <= '9') f |= TK_DIGIT_START;                   // :347
        c[(size_t)i] = f;
    }
    return c;
}

// ---------------------------------------------------------------- greedy search + result state machine
void Greedy::init(const ModelParams *p, const std::vector<uint8_t> *cls)
{
    P_ = p; cls_ = cls;
    memset(active_, 0, sizeof active_);
    for (int &i : active_id_) i = -1;
    head_ = last_call_head_ = 0;
    conf_k_ = 0; side_ = nullptr; evals_ = 0;
    bias_.reset(); bias_state_ = 0;
    set_lm(nullptr, 0.0f, 0.0f);
    set_search_options(nullptr); first_ms_ = 0;
    emitted_silence_ = true;                       // april_session.c:64
    last_emit_ms_ = 0;
    ctx[0] = ctx[1] = 0;
    ctx_dirty = false;
}

void Greedy::call(int type, size_t count, std::vector<Event> &out)
{
    Event e; e.type = type;
    e.tokens.assign(active_, active_ + count);
    if (conf_k_ && count) {
        e.infos.assign(info_, info_ + count);
        for (size_t i = 0; i < count; ++i) e.tokens[i].reserved = &e.infos[i];
    }
    out.push_back(std::move(e));
}

// the round's side record (Engine::conf_records) as the public struct; without a side record (no device behind this search)
// the values are NaN and n_alt is 0
void Greedy::fill_info(uint64_t eval_index)
{
    AprilxTokenInfo &o = cur_info_;
    memset(&o, 0, sizeof o);
    o.size = (uint32_t)sizeof(AprilxTokenInfo);
    o.eval_index = eval_index;
    const float nan = __builtin_nanf("");
    o.lse = o.token_logprob = o.blank_logprob = nan;
    for (int i = 0; i < 8; ++i) o.alt_id[i] = -1;
    if (!side_) return;
    const ConfRecord &c = *side_;
    o.n_alt = (uint32_t)std::max(0, std::min(c.n_alt, std::min(conf_k_, (int)kConfMaxAlt)));
    o.lse = c.lse;
    if (o.n_alt) o.token_logprob = c.alt_logit[0] - c.lse;
    o.blank_logprob = c.blank_val - c.lse;
    for (uint32_t i = 0; i < o.n_alt; ++i) { o.alt_id[i] = c.alt_id[i]; o.alt_logit[i] = c.alt_logit[i]; }
    side_ = nullptr;
}

void Greedy::push_ctx(int tok) { ctx[0] = ctx[1]; ctx[1] = tok; ctx_dirty = true; }   // :181-196 (context_size == 2)

void Greedy::reset_context_to_blank() { push_ctx(P_->blank_id); push_ctx(P_->blank_id); }   // :432-438

void Greedy::clear_context()
{
    if (ctx[0] == P_->blank_id) return;            // :297 (tests element 0, quirk kept)
    push_ctx(P_->blank_id); push_ctx(P_->blank_id);
}

void Greedy::finalize_all(std::vector<Event> &out)
{
    if (head_ == 0) return;                         // :199-211
    call(APRIL_RESULT_RECOGNITION_FINAL, head_, out);
    last_call_head_ = head_;
    head_ = 0;
}

void Greedy::finalize_before_word(const AprilToken &incoming, std::vector<Event> &out)
{
    if (head_ == 0) return;                         // :213-255
    if (incoming.flags & APRIL_TOKEN_FLAG_WORD_BOUNDARY_BIT) { finalize_all(out); return; }
    size_t start = kMaxActive;
    for (size_t i = head_ - 1; i > 2; --i)
        if (active_[i].flags & APRIL_TOKEN_FLAG_WORD_BOUNDARY_BIT) { start = i; break; }
    if (start == (size_t)kMaxActive) { finalize_all(out); return; }
    call(APRIL_RESULT_RECOGNITION_FINAL, start, out);
    memmove(active_, active_ + start, sizeof(AprilToken) * (head_ - start));
    memmove(active_id_, active_id_ + start, sizeof(int) * (head_ - start));
    if (conf_k_) memmove(info_, info_ + start, sizeof(AprilxTokenInfo) * (head_ - start));
    head_ -= start;
}

void Greedy::emit_silence(std::vector<Event> &out)
{
    if (emitted_silence_) return;                   // :257-268
    emitted_silence_ = true;
    Event e; e.type = APRIL_RESULT_SILENCE;
    out.push_back(std::move(e));
}

bool Greedy::emit_partial(const AprilToken *tok, int tok_id, bool force, std::vector<Event> &out)
{
    if (tok) {                                      // :270-294
        if (!force && last_call_head_ == head_ + 1 && active_id_[head_] == tok_id) return false;
        active_[head_] = *tok;
        active_id_[head_] = tok_id;
        if (conf_k_) info_[head_] = cur_info_;
        ++head_;
    } else if (!force && last_call_head_ == head_) {
        return false;
    }
    call(APRIL_RESULT_RECOGNITION_PARTIAL, head_, out);
    last_call_head_ = head_;
    return true;
}

bool Greedy::on_joint(const JointResult &r, float early_emit, size_t now_ms, std::vector<Event> &out)
{
    const int blank = P_->blank_id;
    int best = r.idx;
    float best_v = r.max_val;
    if (best < 0) { best = blank == 0 ? 1 : 0; best_v = -9999999999.0f; }   // no logit beat the initial value (NaNs)
    const float blank_raw = r.blank_val;
    const float blank_v = has_opt_ ? blank_raw - blank_penalty_ : blank_raw;      // bl' (DESIGN.md section 14); the token's logprob and the record keep the raw value

    const bool cleared = ctx[1] == blank;           // :322
    const bool same = ctx[1] == best;               // :326
    if (same) early_emit = 0.0f;
    bool is_blank = (blank_v - early_emit) > best_v;    // :329-330

    const uint8_t tc = (*cls_)[(size_t)best];
    AprilToken tok;
    tok.token = P_->token((size_t)best);
    tok.logprob = best_v;
    tok.flags = (AprilTokenFlagBits)0;
    tok.time_ms = now_ms;
    tok.reserved = nullptr;
    const uint64_t eval_index = evals_++;
    if (conf_k_) fill_info(eval_index);
    int flags = 0;
    if (tc & TK_WORD_START) flags |= APRIL_TOKEN_FLAG_WORD_BOUNDARY_BIT;
    bool eos = (tc & TK_SENT_END) != 0;
    bool punct = eos || (tc & TK_COMMA);
    if (punct && head_ > 0) {                       // :345-351 "10.0" is not a sentence end
        const uint8_t lc = (*cls_)[(size_t)active_id_[head_ - 1]];
        if ((lc & TK_DIGIT_START) && (tc & TK_DOT)) { eos = false; punct = false; }
    }
    if (eos) flags |= APRIL_TOKEN_FLAG_SENTENCE_END_BIT;
    tok.flags = (AprilTokenFlagBits)flags;
    if (!cleared && punct && !same && best_v > (blank_v - 3.5f)) is_blank = false;   // :356-358

    if (!is_blank) {                                // :361-400
        last_emit_ms_ = now_ms;
        push_ctx(best);
        if (bias_) bias_state_ = bias_->next(bias_state_, best);
        if (lm_) lm_state_ = lm_->next(lm_state_, best);
        bool fin = head_ >= (size_t)(kMaxActive - 1);
        if (head_ > 0 && (flags & APRIL_TOKEN_FLAG_WORD_BOUNDARY_BIT)) {
            AprilToken &prev = active_[head_ - 1];
            const bool prev_eos = ((*cls_)[(size_t)active_id_[head_ - 1]] & TK_SENT_END) != 0;
            if (prev_eos && !(prev.flags & APRIL_TOKEN_FLAG_SENTENCE_END_BIT))
                prev.flags = (AprilTokenFlagBits)(prev.flags | APRIL_TOKEN_FLAG_SENTENCE_END_BIT);
            if (prev_eos) fin = true;
        }
        // the utterance cap U: a word that begins U ms or more after the utterance's first token finalises what came before
        if (has_opt_ && max_utt_ms_ && head_ > 0 && (flags & APRIL_TOKEN_FLAG_WORD_BOUNDARY_BIT) && now_ms - first_ms_ >= (size_t)max_utt_ms_) fin = true;
        if (fin) finalize_before_word(tok, out);
        if (head_ >= (size_t)(kMaxActive - 1)) { LOGE("No room left even after finalizing previous words"); head_ = 0; }
        if (head_ == 0) first_ms_ = now_ms;
        emit_partial(&tok, best, true, out);
        emitted_silence_ = false;
    } else {                                        // :401-426
        const size_t gap = now_ms - last_emit_ms_;
        const float decayed = best_v - (float)gap / 3000.0f;
        const bool confident = !same && decayed > (blank_v - 4.0f);
        bool endpoint;
        if (has_opt_) endpoint = gap >= (size_t)endpoint_ms_;      // the session's own endpoint silence E
        // (without options the literal line, in this shape: tests/mutate_product_state_machine.py edits the text of the next line up to its first brace, which
        // must occur exactly once and must decide for every session without options; folding it into `gap >= endpoint_ms_` breaks that yardstick)
        else if (gap >= 2200) { endpoint = true; } else endpoint = false;
        if (endpoint) {
            finalize_all(out);
            clear_context();
            bias_state_ = 0;
            if (lm_) lm_state_ = lm_->start;
            emit_silence(out);
        } else if (confident) {
            tok.logprob -= 8.0f;
            if (emit_partial(&tok, best, false, out)) --head_;
        } else {
            emit_partial(nullptr, -1, false, out);
        }
    }
    return is_blank;
}

void Greedy::finish_flush(std::vector<Event> &out)
{
    bias_state_ = 0;
    if (lm_) lm_state_ = lm_->start;
    finalize_all(out);
    clear_context();
    emit_silence(out);
}

void FrameBook::append_span(size_t l0, size_t l1, Parts &parts) const
{
    const size_t fsz = fifo.size();
    if (l0 < fsz) parts.emplace_back(fifo.data() + l0, std::min(l1, fsz) - l0);
    if (l1 > fsz) parts.emplace_back(ext + (std::max(l0, fsz) - fsz), l1 - std::max(l0, fsz));
}

FbankFrameDesc FrameBook::write_row(int slot, int pcm_off)
{
    FbankFrameDesc d; d.slot = slot; d.ring_row = head; d.pcm_off = pcm_off;
    head = (head + 1) % ring_frames;
    rows_written += 1;
    avail += 1;
    return d;
}

void FrameBook::compact()
{
    if (lent()) return;                                // positions may point into the lent buffer: settle() does it
    if (segmented()) {
        while (segs.size() > 1 && segs[1].pos <= (int64_t)fifo_pos) segs.pop_front();      // segments frames no longer reach
        const int64_t drop = rs_keep() - in_drop;
        if (drop > 0 && (drop >= 8192 || drop == (int64_t)held())) {
            if (fmt) raw.drop((size_t)drop);
            else fifo.erase(fifo.begin(), fifo.begin() + (long)drop);
            in_drop += drop;
        }
        return;
    }
    if (fifo_pos > 0 && (fifo_pos >= 8192 || fifo_pos == fifo.size())) {
        fifo.erase(fifo.begin(), fifo.begin() + (long)fifo_pos);
        fifo_pos = 0;
    }
}

void FrameBook::absorb_ext()
{
    if (fmt) { raw.absorb(); return; }
    if (!ext) return;
    fifo.insert(fifo.end(), ext, ext + ext_cnt);
    ext = nullptr; ext_cnt = 0;
}

void FrameBook::settle()
{
    if (fmt) {
        const int64_t keep = rs_keep() - in_drop;       // (index into raw's bytes ++ ext)
        if (raw.settle((size_t)keep)) in_drop += keep;
    } else if (ext && rs) {
        const int64_t keep = rs_keep() - in_drop;       // (index into fifo ++ ext)
        if (keep >= (int64_t)fifo.size()) {
            fifo.assign(ext + (keep - (int64_t)fifo.size()), ext + ext_cnt);
            in_drop += keep;
            ext = nullptr; ext_cnt = 0;
        } else {
            absorb_ext();
        }
    } else if (ext) {
        if (fifo_pos >= fifo.size()) {                 // everything older is consumed: the fifo becomes the lent buffer's tail
            const size_t skip = fifo_pos - fifo.size();
            fifo.assign(ext + skip, ext + ext_cnt);
            fifo_pos = 0;
            ext = nullptr; ext_cnt = 0;
        } else {
            absorb_ext();
        }
    }
    compact();
}

void FrameBook::rs_update()
{
    if (!segmented()) return;
    const int64_t total = in_drop + (int64_t)held();
    RsSeg *c = &segs.back();
    if (c->closed) {
        if (total == c->in_start + c->n_in) return;
        RsSeg n;                                       // the first samples after a flush open the next segment behind the flush zeros
        n.pos = c->pos + c->n_out + c->zeros; n.in_start = c->in_start + c->n_in;
        segs.push_back(n);
        c = &segs.back();
    }
    c->n_in = total - c->in_start;
    c->n_out = rs ? resample_avail(c->n_in, rs->L, rs->M, rs->K) : c->n_in;
    rs_end = c->pos + c->n_out;
}

void FrameBook::rs_close()
{
    if (!segmented()) return;
    RsSeg &c = segs.back();
    if (c.closed) return;                              // (nothing was fed since the last flush: an empty segment adds no outputs)
    c.closed = true;
    c.n_out = rs ? resample_total(c.n_in, rs->L, rs->M) : c.n_in;
    rs_end = c.pos + c.n_out + c.zeros;
}

void FrameBook::rs_zeros(int64_t n)
{
    segs.back().zeros += n;
    rs_end += n;
}

int64_t FrameBook::rs_keep() const
{
    size_t i = segs.size() - 1;
    while (i > 0 && segs[i].pos > (int64_t)fifo_pos) --i;
    const RsSeg &g = segs[i];
    const int64_t j = (int64_t)fifo_pos - g.pos;
    int64_t k = g.n_in;
    if (!(g.closed && j >= g.n_out)) k = std::min(g.n_in, std::max<int64_t>(0, rs ? resample_k0(j, rs->L, rs->M) - rs->K + 1 : j));
    return g.in_start + k;
}

void FrameBook::set_input(const ResampleSpec *spec, const InputFormat &f)
{
    // only on an idle session after creation or a completed flush: what frames have not consumed yet is less than a frame of the
    // flush zeros (or nothing), so it carries over as zeros
    const int64_t left = (int64_t)(stream_end() - fifo_pos);
    ext = nullptr; ext_cnt = 0;
    fifo.clear();
    raw.clear(); raw.fbytes = f ? f.frame_bytes : 1;
    segs.clear();
    in_drop = 0;
    if (spec || f) {
        RsSeg z;
        z.pos = (int64_t)fifo_pos; z.closed = true; z.zeros = left;
        segs.push_back(z);
        rs_end = z.pos + left;
    } else {
        fifo.assign((size_t)left, (int16_t)0);
        fifo_pos = 0;
        rs_end = 0;
    }
    rs = spec; fmt = f;
}

// ---------------------------------------------------------------- model
Model::~Model()
{
    for (auto *s : scheds) delete s;
    for (auto *e : engines) delete e;
}

// ---------------------------------------------------------------- scheduler

static int host_helpers()
{
    // default: one helper per 16 hardware threads, 3..8 (measured at 2048 sessions: 8 helpers 10.07 ms per step, 3 helpers 10.59)
    const int hw = (int)std::thread::hardware_concurrency();
    const int n = env_int("APRIL_HOST_THREADS", std::max(3, std::min(8, hw / 16)));
    return n < 0 ? 0 : (n > 32 ? 32 : n);
}

static int env_0_1M(const char *name, int def) { return std::max(0, std::min(1000000, env_int(name, def))); }

Scheduler::Scheduler(Model *m, Engine *e)
    : shift_ms_(m->host.params.frame_shift_ms), eng_(e), stride_ms_(m->host.params.segment_step * m->host.params.frame_shift_ms), pool_(host_helpers())
{
    spin_step_us_ = env_0_1M("APRIL_SPIN_STEP_US", 1000);     // (1 ms: a client that pauses for a barrier or a sync between two feeds finds the thread awake; 100 us until round 3)
    spin_wait_us_ = env_0_1M("APRIL_SPIN_WAIT_US", 3000);
    lm_min_chunks_ = env_0_1M("APRIL_LM_MIN_CHUNKS", 8);
    wave_min_chunks_ = env_0_1M("APRIL_WAVE_MIN_CHUNKS", 2);
    pipeline_depth_ = std::max(1, std::min(2, env_0_1M("APRIL_PIPELINE", 2)));
    thread_ = std::thread([this] { loop(); });
}

static inline void cpu_relax() { __builtin_ia32_pause(); }

// both sides of the hand-over: poll a sequence counter (callers the tick counter done_seq_, the stepping thread work_seq_) until it
// moves away from `seen`, for at most `budget_us`, before sleeping on the condition variable
static void spin_while_unchanged(const std::atomic<uint64_t> &seq, uint64_t seen, int budget_us)
{
    if (budget_us <= 0) return;
    const auto t0 = std::chrono::steady_clock::now();
    while (seq.load(std::memory_order_acquire) == seen) {
        for (int i = 0; i < 64; ++i) cpu_relax();
        if (std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > budget_us) break;
    }
}

Scheduler::~Scheduler()
{
    { std::lock_guard<std::mutex> g(mu_); stop_ = true; }
    cv_work_.notify_all();
    if (thread_.joinable()) thread_.join();
    { std::lock_guard<std::mutex> g(mu_); for (LoopCall *c : calls_) c->done = true; calls_.clear(); }      // (their fn never ran; the model is going away)
    cv_done_.notify_all();
}

void Scheduler::attach(Session *s)
{
    std::lock_guard<std::mutex> g(mu_);
    sessions_.push_back(s);
}

bool Scheduler::detach(Session *s)
{
    std::unique_lock<std::mutex> lk(mu_);
    if (on_loop_thread() && s->busy) {
        // aas_free from inside this session's own asynchronous result handler: the stepping thread would wait for itself
        // (the reference joins its own thread there, src/proc_thread.c:101-116).  Refuse loudly instead of hanging.
        LOGE("aas_free called from inside the session's result handler: not supported, the session is left alive");
        return false;
    }
    s->closing = true;
    cv_done_.wait(lk, [&] { return !s->busy; });
    sessions_.erase(std::remove(sessions_.begin(), sessions_.end(), s), sessions_.end());
    s->inbox.clear(); s->raw_inbox.clear();
    s->borrow_ptr = nullptr; s->borrow_cnt = 0;
    return true;
}

SchedStats Scheduler::stats() { std::lock_guard<std::mutex> g(mu_); return stats_; }

size_t Scheduler::latencies(double *out, size_t cap, bool reset)
{
    std::lock_guard<std::mutex> g(mu_);
    const size_t have = lat_ms_.size(), first = lat_n_ > kLatRing ? (size_t)(lat_n_ % kLatRing) : 0;
    const size_t n = out ? std::min(have, cap) : 0;
    for (size_t i = 0; i < n; ++i) out[i] = lat_ms_[(first + (have - n) + i) % have];      // the newest n, oldest first
    const size_t ret = out ? n : have;
    if (reset) { lat_ms_.clear(); lat_n_ = 0; }
    return ret;
}

bool Scheduler::submit(int n, Session *const *ss, const short *const *pcm, const size_t *counts, bool flush, bool wait, bool borrow, bool bytes)
{
    std::vector<Session *> overflowed;
    std::vector<uint64_t> tickets((size_t)n, 0);
    uint64_t done_seen = 0;
    const auto t_sub = std::chrono::steady_clock::now();
    {
        std::unique_lock<std::mutex> lk(mu_);
        if (bytes && !flush)
            for (int i = 0; i < n; ++i) if (counts[i] % (ss[i]->frame_bytes ? ss[i]->frame_bytes : sizeof(int16_t))) return false;      // a partial frame: nothing is queued
        for (int i = 0; i < n; ++i) {
            Session *s = ss[i];
            if (s->closing) continue;
            if (!flush && !bytes && s->frame_bytes && (counts[i] * sizeof(short)) % s->frame_bytes) {
                LOGE("feed of %zu bytes is not a whole number of the session's %zu-byte frames: dropped", counts[i] * sizeof(short), s->frame_bytes);
                continue;
            }
            if (!s->has_oldest) { s->oldest_submit = t_sub; s->has_oldest = true; }
            if (flush) s->flush_requested = true;
            else {
                // positions: samples, or the frames of a session with a format (the bound below counts frames)
                const size_t unit = s->frame_bytes ? s->frame_bytes : sizeof(int16_t);
                const size_t cnt = s->frame_bytes || bytes ? counts[i] * (bytes ? 1 : sizeof(short)) / unit : counts[i];
                // the reference's ring refuses a push that would make it hold MAX_AUDIO samples or more (src/audio_provider.c:61)
                if (!s->sync_mode && s->queued() + s->borrow_cnt + cnt >= s->ring_limit) { overflowed.push_back(s); continue; }   // april_session.c:482-492
                if (cnt) {
                    if (borrow && !s->borrow_cnt && s->queued() == 0) { s->borrow_ptr = pcm[i]; s->borrow_cnt = cnt; }
                    else if (s->frame_bytes) { const uint8_t *b = reinterpret_cast<const uint8_t *>(pcm[i]); s->raw_inbox.insert(s->raw_inbox.end(), b, b + cnt * unit); }
                    else s->inbox.insert(s->inbox.end(), pcm[i], pcm[i] + cnt);
                }
                s->fed = true;
            }
            tickets[(size_t)i] = ++s->submitted;
        }
        // read while mu_ is still held: the tick that takes this work cannot have ended yet (it needs mu_ to collect it), so a
        // later change of done_seq_ is never missed and the spin below never waits on a counter that has already moved
        done_seen = done_seq_.load(std::memory_order_acquire);
    }
    work_seq_.fetch_add(1, std::memory_order_release);
    cv_work_.notify_one();
    for (Session *s : overflowed) s->handlers.result(s->handlers.userdata, APRIL_RESULT_ERROR_CANT_KEEP_UP, 0, nullptr);
    if (!wait) return true;
    spin_while_unchanged(done_seq_, done_seen, spin_wait_us_);
    std::unique_lock<std::mutex> lk(mu_);
    cv_done_.wait(lk, [&] {
        for (int i = 0; i < n; ++i) if (tickets[(size_t)i] && ss[i]->completed < tickets[(size_t)i] && !ss[i]->closing) return false;
        return true;
    });
    return true;
}

void Scheduler::wait_idle(Session *s)
{
    std::unique_lock<std::mutex> lk(mu_);
    cv_done_.wait(lk, [&] { return s->idle(); });
}

template <class Apply> bool Scheduler::configure(Session *s, Apply apply)
{
    wait_idle(s);
    std::lock_guard<std::mutex> g(mu_);
    return s->settable() && apply();
}

bool Scheduler::set_input_rate(Session *s, const ResampleSpec *spec)
{
    return configure(s, [&] {
        s->fb.set_rate(spec);
        s->ring_limit = spec ? (size_t)(48000ull * spec->in_rate / spec->out_rate) : 48000;
        return true;
    });
}

bool Scheduler::set_input_format(Session *s, const InputFormat &f)
{
    return configure(s, [&] {
        s->fb.set_input(s->fb.rs, f);
        s->frame_bytes = f.frame_bytes;
        return true;
    });
}

bool Scheduler::set_confidence(Session *s, int k)
{
    return configure(s, [&] {
        if (k == s->greedy.confidence()) return true;
        s->greedy.set_confidence(k);
        eng_->set_slot_confidence(s->slot, k);          // (queued: the stepping thread applies it before the session's next flight)
        return true;
    });
}

bool Scheduler::set_search_options(Session *s, const AprilxSearchOptions *o)
{
    return configure(s, [&] {
        s->greedy.set_search_options(o);
        // (queued: the stepping thread applies it before the session's next flight; U is the host's alone)
        eng_->set_slot_search_options(s->slot, o ? SearchOpt{o->endpoint_silence_ms, o->blank_penalty} : SearchOpt{0u, 0.0f});
        return true;
    });
}

template <class Obs, class Opt, class Plan, class Handler>
bool Scheduler::set_observer(Session *s, Obs Session::*obs, Handler Handlers::*slot, void *Handlers::*slot_userdata, const Opt *o, const Plan *plan, Handler handler, void *userdata)
{
    return configure(s, [&] {
        Obs &x = s->*obs;
        x = Obs();
        if (plan) { x.on = true; x.opt = *o; x.plan = *plan; }
        s->handlers.*slot = plan ? handler : nullptr; s->handlers.*slot_userdata = plan ? userdata : nullptr;
        return true;
    });
}
bool Scheduler::set_vad(Session *s, const VadOptions *o, const VadPlan *plan, AprilxVadHandler handler, void *userdata) { return set_observer(s, &Session::vad, &Handlers::vad, &Handlers::vad_userdata, o, plan, handler, userdata); }
bool Scheduler::set_dtmf(Session *s, const DtmfOptions *o, const DtmfPlan *plan, AprilxDtmfHandler handler, void *userdata) { return set_observer(s, &Session::dtmf, &Handlers::dtmf, &Handlers::dtmf_userdata, o, plan, handler, userdata); }
bool Scheduler::set_tones(Session *s, const ToneOptions *o, const TonePlan *plan, AprilxToneHandler handler, void *userdata) { return set_observer(s, &Session::tones, &Handlers::tone, &Handlers::tone_userdata, o, plan, handler, userdata); }
bool Scheduler::set_quality(Session *s, const QualityOptions *o, const QualityPlan *plan, AprilxQualityHandler handler, void *userdata) { return set_observer(s, &Session::quality, &Handlers::quality, &Handlers::quality_userdata, o, plan, handler, userdata); }

bool Scheduler::set_bias(Session *s, std::shared_ptr<const BiasSet> set)
{
    return configure(s, [&] {
        if (set.get() == s->greedy.bias() && s->greedy.bias_state() == 0) return true;
        if (!eng_->set_slot_bias(s->slot, set)) return false;      // (queued: the stepping thread applies it before the session's next flight)
        s->greedy.set_bias(std::move(set));
        return true;
    });
}

bool Scheduler::set_lm(Session *s, std::shared_ptr<const LmSet> lm, float weight, float token_bonus)
{
    return configure(s, [&] {
        if (!eng_->set_slot_lm(s->slot, lm, weight, token_bonus)) return false;      // (queued: the stepping thread applies it before the session's next flight)
        s->greedy.set_lm(std::move(lm), weight, token_bonus);
        return true;
    });
}

void Scheduler::wait_idle_many(Session *const *ss, int n)
{
    auto all_idle = [&] {
        for (int i = 0; i < n; ++i) if (!ss[i]->idle()) return false;
        return true;
    };
    std::unique_lock<std::mutex> lk(mu_);
    if (!all_idle()) {   // called right after a submit: poll for the end of the tick that took the work before sleeping
        const uint64_t seen = done_seq_.load(std::memory_order_acquire);      // under the lock, as in submit()
        lk.unlock();
        spin_while_unchanged(done_seq_, seen, spin_wait_us_);
        lk.lock();
    }
    cv_done_.wait(lk, all_idle);
}

void Scheduler::wait_backlog(Session *const *ss, int n, uint64_t max_open)
{
    auto ok = [&] {
        for (int i = 0; i < n; ++i) { const Session *s = ss[i]; if (!s->closing && s->submitted - s->completed > max_open) return false; }
        return true;
    };
    for (;;) {
        uint64_t seen;
        {
            std::lock_guard<std::mutex> g(mu_);
            if (ok()) return;
            seen = done_seq_.load(std::memory_order_acquire);      // under the lock, as in submit()
        }
        spin_while_unchanged(done_seq_, seen, spin_wait_us_);
        if (done_seq_.load(std::memory_order_acquire) != seen) continue;
        std::unique_lock<std::mutex> lk(mu_);
        cv_done_.wait(lk, [&] { return ok() || done_seq_.load(std::memory_order_acquire) != seen; });
    }
}

void deliver_events(std::vector<Event> &ev, const Handlers &to)
{
    for (auto &e : ev) {
        if (e.type >= kQualityEventBase) { if (to.quality && e.quality) to.quality(to.quality_userdata, reinterpret_cast<const AprilxQualityEvent *>(e.quality.get())); }
        else if (e.type >= kToneEventBase) { if (to.tone) to.tone(to.tone_userdata, e.type - kToneEventBase, e.f1, e.f2, e.time_ms); }
        else if (e.type >= kDtmfEventBase) { if (to.dtmf) to.dtmf(to.dtmf_userdata, e.type - kDtmfEventBase, e.digit, e.time_ms); }
        else if (e.type >= kVadEventBase) { if (to.vad) to.vad(to.vad_userdata, e.type - kVadEventBase, e.time_ms); }
        else to.result(to.userdata, (AprilResultType)e.type, e.tokens.size(), e.tokens.empty() ? nullptr : e.tokens.data());
    }
    ev.clear();
}

void Scheduler::deliver_sync_events(Session *s)
{
    std::vector<Event> ev;
    { std::lock_guard<std::mutex> g(mu_); ev.swap(s->done_events); }
    if (ev.empty()) return;
    s->delivering_tid = std::this_thread::get_id();
    s->delivering.store(true, std::memory_order_release);
    deliver_events(ev, s->handlers);
    s->delivering.store(false, std::memory_order_release);
}

bool Scheduler::run_on_loop(const std::function<void()> &fn)
{
    if (on_loop_thread()) return false;
    LoopCall call{&fn};
    std::unique_lock<std::mutex> lk(mu_);
    if (stop_) return false;
    calls_.push_back(&call);
    calls_waiting_.store((int)calls_.size(), std::memory_order_release);
    work_seq_.fetch_add(1, std::memory_order_release);
    cv_work_.notify_one();
    cv_done_.wait(lk, [&] { return call.done; });
    return true;
}

// One stepping thread, TWO flights in the air.  A flight is launched (frames cut, chunk steps enqueued, record copy + event
// queued: launch_flight) without waiting for the GPU; it is completed (wait for its event, replay the records through the
// search state machine, deliver the callbacks, release the callers: complete_flight) AFTER the next flight has been launched
// whenever work for that next flight is already queued -- asynchronous sessions, pipelined group feeds
// (aprilx_feed_many_pipelined), or simply other clients' sessions.  The host part of flight k + 1 (framing, PCM staging, index
// blocks, launch) then runs under the GPU time of flight k instead of between two flights (measured at 256 sessions: 170 us of
// GPU idle time per 100 ms feed, profiles/r04a_b256_timeline.txt).  A caller that blocks on its own feed (aas_feed_pcm16 of a
// synchronous session, aprilx_feed_many) sees the same thing as before: its tickets complete when its flight does.
bool Scheduler::collect(std::vector<Session *> &work, std::vector<uint64_t> &taken, bool block, uint64_t &work_seen)
{
    work.clear(); taken.clear();
    if (block) spin_while_unchanged(work_seq_, work_seen, spin_step_us_);      // a feed usually follows the previous one within microseconds
    Lap lap;
    std::unique_lock<std::mutex> lk(mu_);
    auto have = [&] {
        for (Session *s : sessions_) if (!s->closing && (s->fed || s->flush_requested)) return true;
        return false;
    };
    if (block) cv_work_.wait(lk, [&] { return stop_ || have() || !calls_.empty(); });
    if (!calls_.empty()) { work_seen = work_seq_.load(std::memory_order_acquire); return false; }      // run_on_loop() requests go first (loop())
    work_seen = work_seq_.load(std::memory_order_acquire);
    if (stop_) return false;
    lap();
    collect_has_sub_ = false;
    for (Session *s : sessions_) {
        if (s->closing || (!s->fed && !s->flush_requested)) continue;
        if (s->has_oldest) { if (!collect_has_sub_ || s->oldest_submit < collect_t_sub_) collect_t_sub_ = s->oldest_submit; collect_has_sub_ = true; s->has_oldest = false; }
        s->busy = true;
        s->inflight += 1;
        if (s->borrow_cnt && s->frame_bytes) {
            const uint8_t *b = reinterpret_cast<const uint8_t *>(s->borrow_ptr);
            RawFifo &raw = s->fb.raw;
            if (s->raw_inbox.empty() && !raw.ext) { raw.ext = b; raw.ext_cnt = s->borrow_cnt; }      // read in place during this tick
            else { raw.absorb(); raw.append(b, s->borrow_cnt); }
            s->borrow_ptr = nullptr; s->borrow_cnt = 0;
        } else if (s->borrow_cnt) {
            if (s->inbox.empty() && !s->fb.ext) { s->fb.ext = s->borrow_ptr; s->fb.ext_cnt = s->borrow_cnt; }   // read in place during this tick
            else { s->fb.absorb_ext(); s->fb.fifo.insert(s->fb.fifo.end(), s->borrow_ptr, s->borrow_ptr + s->borrow_cnt); }   // something queued behind it: keep the order
            s->borrow_ptr = nullptr; s->borrow_cnt = 0;
        }
        if (!s->inbox.empty()) { s->fb.absorb_ext(); s->fb.fifo.insert(s->fb.fifo.end(), s->inbox.begin(), s->inbox.end()); s->inbox.clear(); }
        if (!s->raw_inbox.empty()) { s->fb.raw.absorb(); s->fb.raw.append(s->raw_inbox.data(), s->raw_inbox.size() / s->frame_bytes); s->raw_inbox.clear(); }
        if (s->fb.segmented()) s->fb.rs_update();
        if (s->fed) { s->was_flushed = false; s->seg_open = true; }         // april_session.c:510
        s->fed = false;
        if (s->flush_requested) {                                           // :547-552
            s->flush_requested = false;
            if (!s->was_flushed && s->flush_phase == 0) { s->was_flushed = true; s->flush_phase = 1; s->fb.rs_close(); }
            s->seg_open = false;
        }
        work.push_back(s);
        taken.push_back(s->submitted);
    }
    // lent PCM: the caller is blocked until `completed` moves, so its buffer is read in place while the flight is launched (a
    // lent buffer is only accepted when nothing is queued in front of it, so the order of samples is kept)
    tick_.host_ms[0] += lap();
    return !work.empty();
}

// Everything of a tick that does not need the GPU's answers.  Returns the flight (parity -1: nothing reached the GPU).
// final == false: the flight's rings filled up; the same sessions continue in the next flight (loop() keeps `work`).
Scheduler::Flight Scheduler::launch_flight(const std::vector<Session *> &work_in, const std::vector<uint64_t> &taken)
{
    Flight f;
    f.work = work_in; f.taken = taken; f.t0 = std::chrono::steady_clock::now();
    f.t_sub = collect_t_sub_; f.has_sub = collect_has_sub_;      // (a follow-up flight of the same tick keeps the tick's hand-over time)
    f.seq = ++flight_seq_;
    std::vector<Session *> &work = f.work;
    f.mark.resize(work.size()); f.chunks0.resize(work.size());
    for (size_t i = 0; i < work.size(); ++i) { f.mark[i] = (uint32_t)work[i]->replay.size(); f.chunks0[i] = work[i]->chunks; }
    std::vector<Session *> ready;
    eng_->begin_flight();
    bool more = false, any = false;
    const uint64_t steps0 = tick_.steps;
    for (;;) {
        bool progressed = false;
        cut_frames(work, progressed);
        ready.clear();
        for (Session *s : work) if (s->fb.chunk_ready()) ready.push_back(s);
        if (!ready.empty()) {
            if (!step_chunks(ready)) { more = true; break; }          // rings full: land this flight, continue in the next
            progressed = true;
        }
        if (!progressed) break;
        any = true;
    }
    if (more && !any && tick_.steps == steps0) {
        // a step that does not fit an EMPTY flight will never fit: the engine's index / record rings must hold max_batch rows
        // (engine.cc sizes them so); without this the stepping thread would open flight after flight forever
        LOGE("scheduler: a chunk step does not fit an empty flight (index / record rings smaller than one step of max_batch rows)");
        abort();
    }
    Lap lap;
    f.parity = eng_->close_flight();
    f.final = !more;
    for (size_t i = 0; i < work.size(); ++i) f.mark[i] = (uint32_t)work[i]->replay.size() - f.mark[i];      // items this flight appended
    // lent buffers go back to their callers when the tick completes; they are not read after this point (the samples are in
    // pinned staging): keep what framing has not consumed yet
    if (f.final) pool_.run(work.size(), 64, [&](size_t i) { work[i]->fb.settle(); });
    f.chunks1.resize(work.size());
    for (size_t i = 0; i < work.size(); ++i) f.chunks1[i] = work[i]->chunks;
    tick_.host_ms[3] += lap();
    tick_.flights++;
    return f;
}

void Scheduler::complete_flight(Flight &f)
{
    Lap lap;
    eng_->wait_flight(f.parity);
    tick_.host_ms[4] += lap();
    harvest(f.seq);                 // (in front of the flight's token events: no later than the chunks that hold the frames)
    replay(f);
    tick_.host_ms[5] += lap();
    std::vector<Session *> &work = f.work;
    {   // reference src/april_session.c:456-462: EMA of (processing time x 1.1) / audio time per chunk.  All sessions of a
        // flight are stepped together, so a chunk's processing time is the flight's wall time over the chunks the session advanced.
        // With two flights in the air a flight's wall time since its launch includes the time it queued behind the one before it:
        // what it cost is the span since that one completed (the EMA read up to 2 x too high under steady pipelined load)
        const auto now = std::chrono::steady_clock::now();
        const auto from = (have_prev_done_ && prev_done_ > f.t0) ? prev_done_ : f.t0;
        const double tick_ms = std::chrono::duration<double, std::milli>(now - from).count();
        prev_done_ = now; have_prev_done_ = true;
        const double stride_ms = (double)stride_ms_;
        for (size_t i = 0; i < work.size(); ++i) {
            Session *s = work[i];
            const uint64_t n = f.chunks1[i] - f.chunks0[i];
            if (!n) continue;
            double v = s->speed_needed.load(std::memory_order_relaxed);
            for (uint64_t k = 0; k < n; ++k) v = (v * 9.0 + (tick_ms / (double)n) * 1.1 / stride_ms) / 10.0;
            s->speed_needed.store(v, std::memory_order_relaxed);
        }
    }
    // async sessions: deliver on this (library) thread, outside the lock
    for (Session *s : work) if (!s->sync_mode) deliver_events(s->events, s->handlers);
    {
        std::lock_guard<std::mutex> g(mu_);
        for (size_t i = 0; i < work.size(); ++i) {
            Session *s = work[i];
            if (s->sync_mode) { for (auto &e : s->events) s->done_events.push_back(std::move(e)); s->events.clear(); }
            if (f.final) {
                if (f.taken[i] > s->completed) s->completed = f.taken[i];
                s->inflight -= 1;
                s->busy = s->inflight > 0;
            }
        }
        if (f.final) tick_.ticks++;
        if (f.final && f.has_sub) {
            const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - f.t_sub).count();
            if (lat_ms_.size() < kLatRing) lat_ms_.push_back(ms); else lat_ms_[(size_t)(lat_n_ % kLatRing)] = ms;
            ++lat_n_;
        }
        tick_.host_ms[7] += lap();
        stats_.add(tick_);
        tick_ = SchedStats();
    }
    done_seq_.fetch_add(1, std::memory_order_release);
    cv_done_.notify_all();
}

void Scheduler::loop()
{
    HIP_CHECK(hipSetDevice(eng_->device()));
    { std::lock_guard<std::mutex> g(mu_); loop_tid_ = std::this_thread::get_id(); }
    std::vector<Session *> work;
    std::vector<uint64_t> taken;
    uint64_t work_seen = 0;
    bool have_pending = false, have_next = false, cont = false;
    Flight pending, next;
    for (;;) {
        // ---- run_on_loop() requests: between flights.  Whatever is in the air lands first (a tick that continues in a next flight ends first);
        // nothing is launched until the requests have run
        if (!cont && calls_waiting_.load(std::memory_order_acquire)) {
            if (have_pending) { complete_flight(pending); have_pending = false; }
            if (have_next) { complete_flight(next); next = Flight(); have_next = false; }
            std::vector<LoopCall *> todo;
            { std::lock_guard<std::mutex> g(mu_); todo.swap(calls_); calls_waiting_.store(0, std::memory_order_release); }
            for (LoopCall *c : todo) (*c->fn)();
            { std::lock_guard<std::mutex> g(mu_); for (LoopCall *c : todo) c->done = true; }
            cv_done_.notify_all();
        }
        // ---- launch: the continuation of a tick whose flight filled the rings first, else whatever has been queued
        if (!have_next) {
            bool go = cont;
            if (!go) {
                go = collect(work, taken, /*block=*/!have_pending, work_seen);
                if (!go && !have_pending) { std::lock_guard<std::mutex> g(mu_); if (stop_) return; }
            }
            if (go) {
                // a flight launched behind one that is still in the air overlaps with it (and, with steady pipelined feeding, the
                // one after it will be launched behind this one): worth its three streams.  `split_sticky_` keeps the choice for
                // a few flights so that a flight that happened to find the GPU idle does not flip the launch path back and forth
                if (have_pending) split_sticky_ = 8; else if (split_sticky_ > 0) --split_sticky_;
                eng_->set_overlap_hint(pipeline_depth_ >= 2 && split_sticky_ > 0);
                next = launch_flight(work, taken);
                have_next = true;
                cont = !next.final;
            }
        }
        // ---- complete the older flight: at once when a younger one is already behind it on the stream (or nothing can be
        // overlapped: profiling runs account every launch to the flight that issued it), else as soon as the GPU is through
        // with it -- while watching for new work that could still be launched behind it
        if (have_pending) {
            bool done = have_next || pipeline_depth_ < 2 || eng_->profiling();
            if (!done) {
                const auto t0 = std::chrono::steady_clock::now();
                for (;;) {
                    if (eng_->flight_done(pending.parity)) { done = true; break; }
                    if (work_seq_.load(std::memory_order_acquire) != work_seen) break;                 // something was queued: try to launch it first
                    for (int i = 0; i < 32; ++i) cpu_relax();
                    if (std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > spin_wait_us_) { done = true; break; }   // long flight: sleep on it
                }
            }
            if (done) { complete_flight(pending); have_pending = false; }
        }
        if (!have_pending && have_next) {
            pending = std::move(next); next = Flight(); have_next = false; have_pending = true;
            // nothing to overlap with: finish it right away when pipelining is off
            if (pipeline_depth_ < 2 || eng_->profiling()) { complete_flight(pending); have_pending = false; }
        }
    }
}

// A resampled session's window [first, last_end) (model-rate positions): its staging region at `base` is only reserved; per segment it
// overlaps, one resample descriptor and the input span its outputs read (K samples of filter support on each side, clipped to the
// segment) are appended.  Frames overlap, so outputs near a window's edges are computed again in the next window: an output is a pure
// function of the segment's samples, the values are the same.
void Scheduler::stage_resampled(const FrameBook &fb, int64_t first, int64_t last_end, size_t base, size_t &staged_in)
{
    const ResampleSpec &r = *fb.rs;
    pcm_parts_.emplace_back(nullptr, (size_t)(last_end - first));
    for (size_t si = 0; si < fb.segs.size(); ++si) {
        const FrameBook::RsSeg &g = fb.segs[si];
        const int64_t lo = std::max(first, g.pos);
        const int64_t hi = si + 1 < fb.segs.size() ? std::min(last_end, fb.segs[si + 1].pos) : last_end;
        if (lo >= hi) continue;
        ResampleDesc d;
        d.L = r.L; d.M = r.M; d.K = r.K; d.ldt = r.ldt;
        d.out_first = lo - g.pos; d.out_cnt = (int32_t)(hi - lo); d.out_end = g.n_out;
        d.out_dst = (int32_t)(base + (size_t)(lo - first));
        int64_t k_lo = 0, k_hi = 0;
        const int64_t jb = std::min(hi - g.pos, g.n_out);
        if (d.out_first < jb) {
            k_lo = std::max<int64_t>(0, resample_k0(d.out_first, r.L, r.M) - r.K + 1);
            k_hi = std::min<int64_t>(g.n_in, resample_k0(jb - 1, r.L, r.M) + r.K + 1);
        }
        d.in_base = k_lo; d.in_n = (int32_t)std::max<int64_t>(0, k_hi - k_lo); d.in_off = (int32_t)staged_in;
        if (d.in_n > 0) {
            const size_t l0 = (size_t)(g.in_start + k_lo - fb.in_drop);
            if (fb.fmt) {                              // the span is only reserved: the decode launch fills it
                in_parts_.emplace_back(nullptr, (size_t)d.in_n);
                stage_raw(fb, l0, d.in_n, d.in_n, (int32_t)staged_in, true);
            } else fb.append_span(l0, l0 + (size_t)d.in_n, in_parts_);
            staged_in += (size_t)d.in_n;
        }
        rdesc_.push_back(d);
        rspec_.push_back(fb.rs);
    }
}

// Frames [l0, l0 + n_src) of a formatted session's raw queue go into the raw staging region, on a 4-byte boundary (DecodeDesc's
// contract), and one decode descriptor writes out_cnt int16 at `dst`: the decoded frames, then zeros.
void Scheduler::stage_raw(const FrameBook &fb, size_t l0, int32_t n_src, int32_t out_cnt, int32_t dst, bool dst_in)
{
    const size_t pad = (4 - staged_raw_ % 4) % 4;
    if (pad) { raw_parts_.emplace_back(nullptr, pad); staged_raw_ += pad; }
    DecodeDesc d;
    d.src_off = (int64_t)staged_raw_; d.dst = dst; d.out_cnt = out_cnt; d.n_src = n_src;
    d.encoding = (uint8_t)fb.fmt.encoding; d.channels = (uint8_t)fb.fmt.channels; d.channel = (int8_t)fb.fmt.channel; d.dst_in = dst_in ? 1 : 0;
    if (n_src > 0) {
        fb.raw.span(l0, l0 + (size_t)n_src, raw_parts_);
        staged_raw_ += (size_t)n_src * fb.fmt.frame_bytes;
    }
    ddesc_.push_back(d);
}

// A formatted session's window [first, last_end) at the model's rate: its staging region at `base` is only reserved; per segment it
// overlaps, one decode descriptor fills it -- the segment's frames, then the flush zeros behind them.
void Scheduler::stage_decoded(const FrameBook &fb, int64_t first, int64_t last_end, size_t base)
{
    pcm_parts_.emplace_back(nullptr, (size_t)(last_end - first));
    for (size_t si = 0; si < fb.segs.size(); ++si) {
        const FrameBook::RsSeg &g = fb.segs[si];
        const int64_t lo = std::max(first, g.pos);
        const int64_t hi = si + 1 < fb.segs.size() ? std::min(last_end, fb.segs[si + 1].pos) : last_end;
        if (lo >= hi) continue;
        const int64_t j0 = lo - g.pos, jb = std::min(hi - g.pos, g.n_out);
        stage_raw(fb, (size_t)std::max<int64_t>(0, g.in_start + j0 - fb.in_drop), (int32_t)std::max<int64_t>(0, jb - j0), (int32_t)(hi - lo),
                  (int32_t)(base + (size_t)(lo - first)), false);
    }
}

void Scheduler::cut_frames(std::vector<Session *> &work, bool &progressed)
{
    Lap lap;
    desc_.clear(); pcm_parts_.clear(); in_parts_.clear(); rdesc_.clear(); rspec_.clear(); ddesc_.clear(); raw_parts_.clear(); staged_raw_ = 0;
    vdesc_.clear(); tdesc_.clear(); ndesc_.clear(); qdesc_.clear();
    PassPending rec;                            // this pass's record in the pass queue: its runs and flush markers, then its block
    rec.flight = flight_seq_;
    PassFrames obs_frames{};                    // records of this pass's output so far, per observer
    int32_t quality_hop = 0;                    // the hop of the plans behind the quality descriptors
    // one more run of observer o: the `cut` real frames just cut for s, at the next free records of the observer's part (returned)
    auto add_run = [&](Observer o, Session *s, int cut) {
        const int32_t off = (int32_t)obs_frames[o];
        rec.runs[o].push_back(PassRun{s, s->real_frames, cut, off});
        obs_frames[o] += (size_t)cut;
        return off;
    };
    size_t staged = 0, staged_in = 0;           // model-rate samples (windows), input-rate samples (spans of resampled windows)
    auto used = [&] { return staged + staged_in + (staged_raw_ + 1) / 2; };      // what the pass has staged so far, raw bytes of formatted sessions in sample units
    std::vector<Session *> finishers;
    // FbankFrameDesc::pcm_off is a 32-bit sample offset into ONE staging buffer: a pass stages at most `stage_limit` samples
    // (default 2^30; 1640 sessions x a full 8192-frame ring of backlog would pass 2^31) and carries the rest to the next pass
    // of launch_flight()'s loop.  APRIL_STAGE_LIMIT_SAMPLES exists for the test that crosses the limit with small numbers.
    static const size_t stage_limit = [] {
        const char *v = env_str("APRIL_STAGE_LIMIT_SAMPLES");
        const long n = v ? atol(v) : (1L << 30);
        return (size_t)std::min(1L << 30, std::max(1L << 12, n));
    }();
    for (Session *s : work) {
        FrameBook &fb = s->fb;
        // new real frames: frame k covers stream samples [k*shift, k*shift + padded)  (fbank.c:195-236)
        if (fb.can_cut()) {
            // what a window of c frames stages: its model-rate samples, for a resampled session at most this many input samples, and for
            // a formatted session the raw bytes of the one or the other (in sample units, with the spans' alignment)
            auto need = [&](int c) {
                const size_t m = (size_t)(c - 1) * fb.shift + (size_t)fb.padded;
                const size_t in = fb.rs ? (m * fb.rs->M + fb.rs->L - 1) / fb.rs->L + 1 + 3 * (2 * (size_t)fb.rs->K + 2) : 0;
                return m + in + (fb.fmt ? ((fb.rs ? in : m) * fb.fmt.frame_bytes + 1) / 2 + 8 : 0);
            };
            // (an empty pass always takes a frame: a frame that passes the limit alone would otherwise never be staged)
            const size_t used0 = used();
            if (used0 && used0 + need(1) > stage_limit) { progressed = true; continue; }      // next pass
            const size_t base = staged;
            const size_t first = fb.fifo_pos;
            int cut = 0;
            // (up to a ring's worth per pass: a long feed then yields ~70 chunks per session at once for the layer-major step)
            while (fb.can_cut() && cut < fb.ring_frames && ((!used0 && !cut) || used0 + need(cut + 1) <= stage_limit)) {
                desc_.push_back(fb.write_row(s->slot, (int)(base + (size_t)cut * fb.shift)));
                fb.avail_shadow = fb.avail;                       // fbank.c:300
                fb.fifo_pos += (size_t)fb.shift;
                ++cut;
            }
            const size_t last_end = first + (size_t)(cut - 1) * fb.shift + (size_t)fb.padded;
            if (fb.rs) stage_resampled(fb, (int64_t)first, (int64_t)last_end, base, staged_in);
            else if (fb.fmt) stage_decoded(fb, (int64_t)first, (int64_t)last_end, base);
            else fb.append_span(first, last_end, pcm_parts_);                 // (contiguous in staging)
            staged += last_end - first;
            const int32_t first_desc = (int32_t)(desc_.size() - (size_t)cut);      // the run's frame descriptors are the last `cut` of this pass
            if (s->vad.on) {                           // the run of real rows just cut: one descriptor, one byte per row
                VadDesc v;
                v.slot = s->slot; v.first_row = desc_[(size_t)first_desc].ring_row; v.n = cut; v.out_off = add_run(OBS_VAD, s, cut);
                v.flags = s->vad.reset ? VAD_RESET : 0; v.plan = s->vad.plan;
                vdesc_.push_back(v);
                s->vad.reset = false;
            }
            if (s->dtmf.on) {
                DtmfDesc t;
                t.first = first_desc; t.n = cut; t.out_off = add_run(OBS_DTMF, s, cut); t.plan = s->dtmf.plan;
                tdesc_.push_back(t);
            }
            if (s->tones.on) {
                ToneDesc t;
                t.first = first_desc; t.n = cut; t.out_off = add_run(OBS_TONE, s, cut); t.plan = s->tones.plan;
                ndesc_.push_back(t);
            }
            if (s->quality.on) {
                QualityDesc q;
                q.first = first_desc; q.n = cut; q.out_off = add_run(OBS_QUALITY, s, cut); q.clip_level = s->quality.plan.clip_level;
                qdesc_.push_back(q);
                quality_hop = s->quality.plan.hop;
            }
            s->real_frames += (uint64_t)cut;
            s->compact_pending = true;                 // the fifo must not move until the window has been staged
            progressed = true;
            continue;
        }
        if (fb.chunk_ready() || s->flush_phase == 0) continue;
        // drained: flush state machine (april_session.c:552-563, fbank.c:308-325)
        switch (s->flush_phase) {
        case 1: case 3:
            if (fb.flush_allowed()) {
                // The reference drains with "pad the ring up to one segment, pull it, ask again" (src/fbank.c:308-325 under
                // src/april_session.c:552-560) until the shadow counter says stop.  Every round pads exactly what the pull before it
                // consumed and lowers the shadow counter by one segment step, so the number of rounds is known now: all their
                // padding rows go out in this pass and the rounds' chunks are stepped TOGETHER (one wavefront instead of one
                // single-chunk step per round: the 28 flush chunks of a session cost 2 steps instead of 28).  Same rows in the same
                // ring places, same counters afterwards.
                long av = fb.avail, sh = fb.avail_shadow;
                const long floor_sh = -(long)(fb.seg_count * 3);
                const long room = (long)fb.ring_frames - fb.avail;
                long pad = 0;
                while (sh >= floor_sh) {
                    const long need = av < fb.seg_count ? fb.seg_count - av : 0;
                    if (pad + need > room) break;                 // (never with the default ring; a tiny test ring takes the rest next pass)
                    pad += need; av += need;
                    av -= fb.seg_step; sh -= fb.seg_step;
                }
                for (long i = 0; i < pad; ++i) desc_.push_back(fb.write_row(s->slot, -1));     // padding does not touch the shadow counter
            } else {
                s->flush_phase += 1;
            }
            progressed = true;
            break;
        case 2:
            if (fb.segmented()) fb.rs_zeros(2 * 3200);                                // (model-rate zeros behind the closed segment)
            else { fb.absorb_ext(); fb.fifo.insert(fb.fifo.end(), (size_t)2 * 3200, (int16_t)0); }      // april_session.c:555-556
            s->flush_phase = 3;
            progressed = true;
            break;
        case 4:
            // FINAL, clear context, SILENCE (april_session.c:561-563): the host part is replayed in order with the chunk
            // records of this flight; the device part (context reset + decoder refresh) is queued here
            s->replay.push_back(Session::Replay{-1, 0, 0, (uint32_t)s->now_ms, 1, 0});
            finishers.push_back(s);
            // every observer of the session closes what is open (a segment, a held digit or tone, the interval) and starts afresh
            for (int o = 0; o < OBS_COUNT; ++o) if (s->observes(o)) rec.runs[o].push_back(PassRun{s, s->real_frames, -1, 0});
            if (s->vad.on) s->vad.reset = true;
            s->flush_phase = 0;
            progressed = true;
            break;
        default: break;
        }
    }
    tick_.host_ms[1] += lap();
    if (!desc_.empty()) {
        FrontPass pass;
        pass.n_dc = (int)ddesc_.size(); pass.dc = ddesc_.data(); pass.raw_parts = raw_parts_.data(); pass.n_raw_parts = raw_parts_.size(); pass.n_raw = staged_raw_;
        pass.n_rs = (int)rdesc_.size(); pass.rs = rdesc_.data(); pass.rs_specs = rspec_.data(); pass.in_parts = in_parts_.data(); pass.n_in_parts = in_parts_.size(); pass.n_in = staged_in;
        pass.observe(vdesc_.data(), vdesc_.size(), obs_frames[OBS_VAD]); pass.observe(tdesc_.data(), tdesc_.size(), obs_frames[OBS_DTMF]);
        pass.observe(ndesc_.data(), ndesc_.size(), obs_frames[OBS_TONE]); pass.observe(qdesc_.data(), qdesc_.size(), obs_frames[OBS_QUALITY]);
        pass.quality_hop = quality_hop;
        rec.block = eng_->fbank((int)desc_.size(), desc_.data(), pcm_parts_.data(), pcm_parts_.size(), staged, &pool_, pass);
        pool_.run(work.size(), 64, [&](size_t i) { Session *s = work[i]; if (s->compact_pending) { s->fb.compact(); s->compact_pending = false; } });
        tick_.frames += desc_.size();
        tick_.host_ms[2] += lap();
    }
    // the block is lent until this flight has been waited for and harvest() has read it
    rec.at = pass_layout(obs_frames);
    bool runs = false;
    for (int o = 0; o < OBS_COUNT; ++o) runs = runs || !rec.runs[o].empty();
    if (rec.block || runs) pass_pending_.push_back(std::move(rec));
    if (!finishers.empty()) {
        slots_.clear();
        for (Session *s : finishers) slots_.push_back(s->slot);
        eng_->decode_rows((int)slots_.size(), slots_.data(), 1);
        tick_.host_ms[6] += lap();
    }
}

// T consecutive chunks of each of the m sessions of `group` (all have them waiting) as ONE engine step.  STEP_CHUNK: the chunk step
// (T == 1; reference src/april_session.c:431-476, batched).  STEP_LAYER_MAJOR: a long feed ("whole file at once", reference use case
// example.cpp:157-216): the encoder does not depend on emitted tokens, so the T chunks of a session go through each layer together, see
// Engine::lm_step.  STEP_WAVE: the 2..3 chunks of a feed as one wavefront over the layers (Engine::lm_step mode 1).  Row t * m + i of
// the step is chunk t of session i; its three rounds of records (and traced logits) are at (t * 3 + r) * m + i.
bool Scheduler::advance(Session *const *group, int m, int T, StepPath path)
{
    const int rows = m * T;
    const NetDims &d = eng_->dims();
    // (the chunk path's caller has asked for the room of all its sub-batches at once)
    if (path != STEP_CHUNK && !eng_->flight_has_room(rows + m, 1)) return false;
    slots_.clear(); tails_.assign((size_t)rows, 0); now_.assign((size_t)rows, 0);
    bool traced = false;
    for (int i = 0; i < m; ++i) {
        Session *s = group[i];
        FrameBook &fb = s->fb;
        slots_.push_back(s->slot);
        for (int t = 0; t < T; ++t) {
            tails_[(size_t)t * m + i] = (fb.tail + t * fb.seg_step) % fb.ring_frames;          // fbank.c:327-349, T pulls
            now_[(size_t)t * m + i] = (int)(s->now_ms + (size_t)(t + 1) * stride_ms_);        // april_session.c:442-443
        }
        fb.tail = (fb.tail + T * fb.seg_step) % fb.ring_frames;
        fb.avail -= (long)T * fb.seg_step;
        fb.avail_shadow -= (long)T * fb.seg_step;
        if (s->trace_buf) traced = true;
    }
    if (traced) logit_stage_.resize((size_t)3 * rows * d.vocab);
    float *logits = traced ? logit_stage_.data() : nullptr;
    const int k = path == STEP_CHUNK ? eng_->step(m, slots_.data(), tails_.data(), now_.data(), logits)
                                     : eng_->lm_step(m, T, slots_.data(), tails_.data(), now_.data(), logits, path == STEP_WAVE ? 1 : 0);
    for (int i = 0; i < m; ++i) {
        Session *s = group[i];
        for (int t = 0; t < T; ++t) {
            s->now_ms += (size_t)stride_ms_;
            s->chunks++;
            s->replay.push_back(Session::Replay{k, i, m, (uint32_t)s->now_ms, 0, t});
            if (traced && s->trace_buf) {                               // tests: the logits of every round that ran, in order
                const StepRecord *recs = eng_->records(k);
                for (int r = 0; r < 3; ++r) {
                    const size_t at = ((size_t)t * 3 + r) * m + i;
                    const StepRecord &rec = recs[at];
                    if (!(rec.flags & REC_VALID)) break;
                    if (*s->trace_used + (size_t)d.vocab <= s->trace_cap) {
                        memcpy(s->trace_buf + *s->trace_used, logit_stage_.data() + at * d.vocab, (size_t)d.vocab * 4);
                        *s->trace_used += (size_t)d.vocab;
                    }
                    if (rec.flags & REC_BLANK) break;
                }
            }
        }
    }
    tick_.steps++; tick_.chunks += (uint64_t)rows;
    if (path == STEP_WAVE) { tick_.wave_steps++; tick_.wave_chunks += (uint64_t)rows; }
    if (path == STEP_LAYER_MAJOR) { tick_.lm_steps++; tick_.lm_chunks += (uint64_t)rows; }
    if ((uint64_t)m > tick_.max_batch_seen) tick_.max_batch_seen = (uint64_t)m;
    return true;
}

// Who goes where: every ready session advances by at least one chunk, on the path that suits its backlog.
bool Scheduler::step_chunks(std::vector<Session *> &ready)
{
    Lap lap;
    const int MB = eng_->max_batch();
    // first use of a session: context = [blank, blank] (already in the slot's device state), run the decoder (april_session.c:432-438)
    slots_.clear();
    for (Session *s : ready) if (!s->dout_ready) {
        s->greedy.reset_context_to_blank();
        s->greedy.ctx_dirty = false;
        s->dout_ready = true;
        slots_.push_back(s->slot);
    }
    if (!slots_.empty()) { eng_->decode_rows((int)slots_.size(), slots_.data(), 0); tick_.host_ms[6] += lap(); }
    struct Enqueued { Lap &lap; double &ms; ~Enqueued() { ms += lap(); } } enqueued{lap, tick_.host_ms[3]};      // on every way out

    // sessions with a long backlog (a whole file fed at once) go layer-major, in groups that fit the work buffers
    std::vector<Session *> one, lm;
    auto waiting = [](const Session *s) { return (int)((s->fb.avail - s->fb.seg_count) / s->fb.seg_step + 1); };
    // the chunks m sessions can advance together: what the work buffers hold, and what every one of them has waiting
    auto depth = [&](Session *const *g, int m) { int T = MB / m; for (int i = 0; i < m; ++i) T = std::min(T, waiting(g[i])); return T; };
    // (fp16 tile engines: layer-major since round 4 -- the tile kernels have the two halves of the gate GEMM; APRIL_F16_LM=0 falls back
    // to successive feed wavefronts of up to wave_max_chunks_ chunks)
    static const bool f16_lm = env_int("APRIL_F16_LM", 1) != 0;
    const bool lm_ok = lm_min_chunks_ > 0 && lm_min_chunks_ <= MB && (!eng_->f16_tile() || f16_lm);
    for (Session *s : ready) ((lm_ok && waiting(s) >= lm_min_chunks_) ? lm : one).push_back(s);
    // ... a FEW sessions: layer-major pays while the rows of a time step are a handful (the recurrent pair of a step as weight streams,
    // everything else batched over time); from ~48 sessions with a backlog the successive feed wavefronts of up to wave_max_chunks_
    // chunks are faster (aprilv0 dims, 2 .. 10 s handed over at once, ms per 100 ms of all sessions, layer-major vs wavefronts: 1 session
    // 0.13 vs 0.33, 32: 0.33 vs 0.49, 64: 0.73 vs 0.60, 256: 1.74 vs 1.31 -- round 6; an asynchronous client that runs ahead of the GPU
    // is the case: bench.py `reference_api_async` 1.93 -> 1.45 ms per step)
    constexpr size_t lm_max_sessions = 48;
    // (ADVICE.md finding 1, the wavefront depth cliff: the backlog sessions merged here share the depth of the shortest session of `one`)
    if (lm.size() > lm_max_sessions && wave_min_chunks_ > 0) { one.insert(one.end(), lm.begin(), lm.end()); lm.clear(); }
    const int per = lm_ok ? std::max(1, MB / lm_min_chunks_) : 1;
    for (size_t o = 0; o < lm.size(); o += (size_t)per) {
        const int m = (int)std::min(lm.size() - o, (size_t)per);
        if (!advance(lm.data() + o, m, depth(lm.data() + o, m), STEP_LAYER_MAJOR)) return false;
    }

    const int n = (int)one.size();
    if (n == 0) return true;
    // A feed usually carries 2..3 chunks for every session (100 ms = 2.5 chunks): those chunk steps run as ONE wavefront over
    // the layers when the rows fit the work buffers; what is left over goes chunk by chunk, in sub-batches of at most MB sessions.
    if (wave_min_chunks_ > 0) {
        const int T = std::min(depth(one.data(), n), wave_max_chunks_);
        if (T >= wave_min_chunks_) return advance(one.data(), n, T, STEP_WAVE);
    }
    if (!eng_->flight_has_room(n, (n + MB - 1) / MB)) return false;
    for (int o = 0; o < n; o += MB) advance(one.data() + o, std::min(MB, n - o), 1, STEP_CHUNK);
    return true;
}

// After the flight's wait: the bytes of every pass cut under it (and under the flights before it) are on the host.  The records up to
// the flight are walked once per observer, in the block's order -- all VAD runs of all of them, then all DTMF runs, then all tone runs,
// then all quality runs: the order of a session's observer events in front of the flight's token events --, then each gives its block
// back and goes.  The sessions are alive: they stay busy until their flight completes.  A flush marker reaches its observer without
// records; a run of an engine that lent no block to its pass is skipped, by all observers alike; else the observer gets the run's
// records in the block (pinned memory, every part at its alignment: pass_layout.h).
void Scheduler::harvest(uint64_t flight)
{
    size_t n = 0;
    while (n < pass_pending_.size() && pass_pending_[n].flight <= flight) ++n;
    for (int o = 0; o < OBS_COUNT; ++o)
        for (size_t i = 0; i < n; ++i) {
            const PassPending &p = pass_pending_[i];
            for (const PassRun &r : p.runs[o]) {
                if (r.n >= 0 && !p.block) continue;
                const uint8_t *b = r.n < 0 ? nullptr : p.block + p.at.record_at(o, (size_t)r.off);
                switch (o) {
                case OBS_VAD: harvest_vad(r, b); break;
                case OBS_DTMF: harvest_dtmf(r, b); break;
                case OBS_TONE: harvest_tone(r, reinterpret_cast<const uint32_t *>(b)); break;
                default: harvest_quality(r, reinterpret_cast<const uint32_t *>(b)); break;
                }
            }
        }
    for (; n; --n) {
        if (pass_pending_.front().block) eng_->release_pass_block(pass_pending_.front().block);
        pass_pending_.pop_front();
    }
}

// One VAD run: the events that follow from bit 0 of consecutive bytes go to the session's event list; a completed flush closes an open segment.
void Scheduler::harvest_vad(const PassRun &r, const uint8_t *b)
{
    Session *s = r.s;
    auto emit = [&](int kind, uint64_t ms) {
        Event e; e.type = kVadEventBase + kind; e.time_ms = ms;
        s->events.push_back(std::move(e));
        if (kind == VAD_SPEECH_START) s->vad.segments++;
    };
    if (!b) { if (s->vad.last) emit(VAD_SPEECH_END, r.t0 * (uint64_t)shift_ms_); s->vad.last = 0; return; }
    s->vad.last = vad_events(s->vad.plan, shift_ms_, r.t0, b, (size_t)r.n, s->vad.last, emit);
    for (int32_t i = 0; i < r.n; ++i) s->vad.speech += b[i] & 1u;
}

// One DTMF run: the codes of consecutive real frames go through the session's event machine (dtmf.h); a completed flush closes a held digit.
void Scheduler::harvest_dtmf(const PassRun &r, const uint8_t *b)
{
    Session *s = r.s;
    auto emit = [&](int kind, char digit, uint64_t ms) {
        Event e; e.type = kDtmfEventBase + kind; e.time_ms = ms; e.digit = digit;
        s->events.push_back(std::move(e));
        if (kind == DTMF_DOWN) s->dtmf.digits++;
    };
    if (!b) { dtmf_flush(shift_ms_, r.t0, s->dtmf.m, emit); return; }
    dtmf_events(s->dtmf.plan, shift_ms_, r.t0, b, (size_t)r.n, s->dtmf.m, emit);
    for (int32_t i = 0; i < r.n; ++i) s->dtmf.tone += b[i] ? 1u : 0u;
}

// One tone run: the records of consecutive real frames go through the session's event machine (tone.h); a completed flush closes a held tone.
void Scheduler::harvest_tone(const PassRun &r, const uint32_t *b)
{
    Session *s = r.s;
    auto emit = [&](int kind, uint32_t f1, uint32_t f2, uint64_t ms) {
        Event e; e.type = kToneEventBase + kind; e.time_ms = ms; e.f1 = f1; e.f2 = f2;
        s->events.push_back(std::move(e));
        if (kind == TONE_ON) s->tones.tones++;
    };
    if (!b) { tone_flush(shift_ms_, r.t0, s->tones.m, emit); return; }
    tone_events(s->tones.plan, shift_ms_, r.t0, b, (size_t)r.n, s->tones.m, emit);
    for (int32_t i = 0; i < r.n; ++i) s->tones.tonal += (b[i] & 0xffffu) ? 1u : 0u;
}

// One quality run: the records of consecutive real frames go through the session's machine (quality.h); a completed flush closes the open
// interval and whatever is on.
void Scheduler::harvest_quality(const PassRun &r, const uint32_t *b)
{
    Session *s = r.s;
    auto emit = [&](const QualityEvent &q) {
        Event e; e.type = kQualityEventBase + q.kind; e.time_ms = q.time_ms; e.quality.reset(new QualityEvent(q));
        s->events.push_back(std::move(e));
        if (q.kind == QUALITY_REPORT) s->quality.reports++;
    };
    if (!b) { quality_flush(s->quality.plan, shift_ms_, r.t0, s->quality.m, emit); return; }
    quality_events(s->quality.plan, shift_ms_, r.t0, b, (size_t)r.n, s->quality.m, emit);
    for (int32_t i = 0; i < r.n; ++i) {
        const uint32_t *w = b + (size_t)i * kQualityWords;
        s->quality.frames++; s->quality.clip_samples += w[4] & 0xffffu;
        s->quality.clipped += (w[4] >> 16) >= (uint32_t)s->quality.plan.clip_run_min ? 1u : 0u; s->quality.dead += w[5] & 1u;
    }
}

// After the flight: per session, in the order things happened, feed the device's per-round records to the search state
// machine (which builds the callbacks) and check that it takes the same decisions the device took.
void Scheduler::replay(Flight &f)
{
    for (size_t w = 0; w < f.work.size(); ++w) {
        Session *s = f.work[w];
        // the first mark[w] items of the session's list are this flight's (flights complete in the order they were launched)
        const size_t n = f.mark[w];
        for (size_t q = 0; q < n; ++q) {
            const Session::Replay &it = s->replay[q];
            if (it.kind == 1) { s->greedy.finish_flush(s->events); s->greedy.ctx_dirty = false; continue; }
            const StepRecord *recs = eng_->records(it.step);
            const ConfRecord *side = s->greedy.confidence() ? eng_->conf_records(it.step) : nullptr;
            for (int r = 0; r < 3; ++r) {                               // april_session.c:449-454
                const StepRecord &rec = recs[((size_t)it.chunk * 3 + r) * it.rows + it.row];
                if (side) s->greedy.set_side(&side[((size_t)it.chunk * 3 + r) * it.rows + it.row]);
                if (!(rec.flags & REC_VALID)) { tick_.replay_mismatch++; LOGE("replay: device skipped a round the host expected (slot %d)", s->slot); break; }
                const JointResult jr{rec.idx, rec.max_val, rec.blank_val};
                const bool blank = s->greedy.on_joint(jr, r == 0 ? 1.0f : 0.0f, (size_t)it.now_ms, s->events);
                const bool ctx = s->greedy.ctx_dirty;
                s->greedy.ctx_dirty = false;
                tick_.rounds++;
                if (blank != ((rec.flags & REC_BLANK) != 0) || ctx != ((rec.flags & REC_CTX) != 0)) {
                    tick_.replay_mismatch++;
                    LOGE("replay: host and device decisions differ (slot %d, round %d: host blank=%d ctx=%d, device flags=%u)", s->slot, r, (int)blank, (int)ctx, rec.flags);
                }
                if (blank) break;
            }
        }
        s->replay.erase(s->replay.begin(), s->replay.begin() + (long)n);
    }
}

}  // namespace aprilx
