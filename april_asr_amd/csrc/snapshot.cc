// Session snapshot / restore, the engine-facing half: the sessions of a call grouped by scheduler, the idle
// wait, the one gather / scatter per engine on its stepping thread (Scheduler::run_on_loop), and the blob put together from / taken
// apart into the images of snapshot.h.  Kept apart from session.cc: the scheduler harness links that file against an engine of its own.
#include "snapshot.h"
#include <algorithm>
#include <map>
#include "common.h"

namespace aprilx {

namespace {
constexpr uint32_t kAlwaysMask = (1u << Engine::SNAP_H) | (1u << Engine::SNAP_C) | (1u << Engine::SNAP_H16) | (1u << Engine::SNAP_EOUT) | (1u << Engine::SNAP_DOUT) |
                                 (1u << Engine::SNAP_GSTATE) | (1u << Engine::SNAP_RING);
constexpr size_t kDeviceHeader = 16 + 16 * Engine::SNAP_ARRAYS;

uint32_t device_mask(const Session &s)
{
    // a session without a set has no trie state; a detector whose reset flag is set carries the flag and no device state
    return kAlwaysMask | (s.greedy.bias() ? 1u << Engine::SNAP_BIAS : 0u) | (s.vad.on && !s.vad.reset ? 1u << Engine::SNAP_VAD : 0u);
}

// the same from a blob's session block, for the session it is restored into
uint32_t device_mask_of(const snap::SessionImage &m, const Session &target)
{
    return kAlwaysMask | (target.greedy.bias() ? 1u << Engine::SNAP_BIAS : 0u) | (m.vad_on && !m.vad_reset ? 1u << Engine::SNAP_VAD : 0u);
}

uint64_t bias_hash(const BiasSet &b)
{
    uint64_t h = snap::fnv1a(b.state_off.data(), b.state_off.size() * 4);
    h = snap::fnv1a(b.edge_tok.data(), b.edge_tok.size() * 4, h);
    h = snap::fnv1a(b.edge_next.data(), b.edge_next.size() * 4, h);
    return snap::fnv1a(b.edge_bonus.data(), b.edge_bonus.size() * 4, h);
}

void copy_text(char *dst, size_t cap, const std::string &s) { memset(dst, 0, cap); memcpy(dst, s.data(), std::min(cap - 1, s.size())); }

bool fresh(const Session &s)
{
    return s.settable() && s.submitted == s.completed && !s.dout_ready && !s.was_flushed && s.chunks == 0 && s.real_frames == 0 && s.now_ms == 0 &&
           s.fb.rows_written == 0 && s.fb.held() == 0 && s.fb.fifo_pos == 0 && s.greedy.bias_state() == 0;
}

template <typename T> bool same(const T &a, const T &b) { return memcmp(&a, &b, sizeof(T)) == 0; }
}  // namespace

// configuration, identity and progress of an idle session, as the blob's info block stores them
AprilxSnapshotInfo snapshot_info_of(const Session &s)
{
    AprilxSnapshotInfo o;
    memset(&o, 0, sizeof o);
    const Model &m = *s.model;
    const ModelParams &p = m.host.params;
    const NetDims &d = s.eng->dims();
    o.size = (uint32_t)sizeof o; o.version = snap::kVersion;
    const int32_t pv[13] = {p.batch_size, p.segment_size, p.segment_step, p.mel_features, p.sample_rate, p.frame_shift_ms, p.frame_length_ms, p.round_pow2, p.mel_low,
                            p.mel_high, p.snip_edges, p.token_count, p.blank_id};
    o.params_hash = snap::fnv1a(pv, sizeof pv);
    o.token_hash = bias_vocab_hash(p);
    o.chunks = s.chunks; o.frames_seen = s.real_frames; o.now_ms = s.now_ms; o.rows_written = s.fb.rows_written;
    o.n_layers = d.n_layers; o.d_model = d.d_model; o.hidden = d.hidden; o.ffn = d.ffn; o.joiner = d.joiner; o.vocab = d.vocab; o.mel = d.mel;
    o.segment_size = p.segment_size; o.segment_step = p.segment_step; o.sample_rate = p.sample_rate; o.frame_shift_ms = p.frame_shift_ms; o.blank_id = p.blank_id;
    o.precision = (uint32_t)s.eng->precision(); o.f16_tile = s.eng->f16_tile() ? 1u : 0u;
    o.input_rate = s.fb.rs ? s.fb.rs->in_rate : (uint32_t)p.sample_rate;
    o.confidence_k = (uint32_t)s.greedy.confidence();
    o.ring_rows = (uint32_t)std::max(0L, s.fb.avail);
    if (s.fb.fmt) { o.has_format = 1; o.format = AprilxInputFormat{(uint32_t)sizeof(AprilxInputFormat), s.fb.fmt.encoding, s.fb.fmt.channels, s.fb.fmt.channel}; }
    if (s.greedy.has_search_options()) { o.has_search_options = 1; o.search = s.greedy.search_options(); }
    if (s.vad.on) {
        const VadOptions &v = s.vad.opt;
        o.has_vad = 1; o.vad = AprilxVadOptions{(uint32_t)sizeof(AprilxVadOptions), v.band_lo_hz, v.band_hi_hz, v.onset_db, v.offset_db, v.onset_ms, v.hangover_ms, v.min_energy, 0u};
    }
    if (s.dtmf.on) {
        const DtmfOptions &v = s.dtmf.opt;
        o.has_dtmf = 1;
        o.dtmf = AprilxDtmfOptions{(uint32_t)sizeof(AprilxDtmfOptions), v.min_level_dbfs, v.twist_hi_db, v.twist_lo_db, v.rel_peak_db, v.min_share, v.min_tone_ms, v.min_pause_ms, 0u};
    }
    if (s.tones.on) {
        const ToneOptions &v = s.tones.opt;
        o.has_tones = 1; o.tones = AprilxToneOptions{(uint32_t)sizeof(AprilxToneOptions), v.min_level_dbfs, v.second_db, v.min_share, v.tol_hz, v.min_tone_ms, v.min_pause_ms, 0u};
    }
    if (const BiasSet *b = s.greedy.bias()) { o.has_bias = 1; o.bias_flags = b->flags; o.bias_states = b->states(); o.bias_edges = b->edges(); o.bias_hash = bias_hash(*b); }
    copy_text(o.name, sizeof o.name, m.host.name); copy_text(o.description, sizeof o.description, m.host.description);
    return o;
}

// what must agree between a blob and the session it is restored into, one field at a time; null: they agree
const char *snapshot_mismatch(const AprilxSnapshotInfo &b, const AprilxSnapshotInfo &t)
{
    if (b.size != t.size || b.version != t.version) return "info block of another version";
    if (b.n_layers != t.n_layers || b.d_model != t.d_model || b.hidden != t.hidden || b.ffn != t.ffn || b.joiner != t.joiner || b.vocab != t.vocab || b.mel != t.mel)
        return "another model: dimensions differ";
    if (b.params_hash != t.params_hash || b.segment_size != t.segment_size || b.segment_step != t.segment_step || b.sample_rate != t.sample_rate ||
        b.frame_shift_ms != t.frame_shift_ms || b.blank_id != t.blank_id) return "another model: PARAMS differ";
    if (b.token_hash != t.token_hash) return "another model: token list differs";
    if (memcmp(b.name, t.name, sizeof b.name) != 0 || memcmp(b.description, t.description, sizeof b.description) != 0) return "another model: name or description differs";
    if (b.precision != t.precision || b.f16_tile != t.f16_tile) return "another precision";
    if (b.input_rate != t.input_rate) return "configuration differs: input rate";
    if (b.has_format != t.has_format || !same(b.format, t.format)) return "configuration differs: input format";
    if (b.confidence_k != t.confidence_k) return "configuration differs: confidence alternatives";
    if (b.has_search_options != t.has_search_options || !same(b.search, t.search)) return "configuration differs: search options";
    if (b.has_vad != t.has_vad || !same(b.vad, t.vad)) return "configuration differs: voice-activity options";
    if (b.has_dtmf != t.has_dtmf || !same(b.dtmf, t.dtmf)) return "configuration differs: DTMF options";
    if (b.has_tones != t.has_tones || !same(b.tones, t.tones)) return "configuration differs: tone options";
    if (b.has_bias != t.has_bias || b.bias_flags != t.bias_flags || b.bias_states != t.bias_states || b.bias_edges != t.bias_edges || b.bias_hash != t.bias_hash)
        return "configuration differs: bias set";
    return nullptr;
}

// ---------------------------------------------------------------- snapshot
// n sessions of ONE scheduler: out[i] receives the blob, ok[i] whether there is one
static void snapshot_group(Scheduler *sched, Session *const *ss, int n, std::vector<uint8_t> *out, bool *ok, bool sizes_only)
{
    for (int i = 0; i < n; ++i) ok[i] = !sched->in_own_handler(ss[i]);
    // a session with a language model is refused: the format does not carry the model's node (DESIGN.md sections 19 and 20)
    for (int i = 0; i < n; ++i) if (ss[i]->greedy.lm()) { ok[i] = false; LOGW("snapshot: refused: the session has a language model, whose node a snapshot does not carry"); }
    // ... and so is a session with the line-quality observer: the format does not carry its machine
    for (int i = 0; i < n; ++i) if (ss[i]->quality.on) { ok[i] = false; LOGW("snapshot: refused: the session has the line-quality observer on, whose machine a snapshot does not carry"); }
    if (sched->on_loop_thread()) return;                       // (a handler on the stepping thread: it would wait for itself)
    sched->submit(0, nullptr, nullptr, nullptr, false, false);   // wake-up only (aprilx_session_drain)
    sched->wait_idle_many(ss, n);
    Engine *eng = sched->engine();
    const Engine::SnapLayout lay = eng->snapshot_layout();
    std::vector<std::vector<uint8_t>> blocks((size_t)n * snap::B_COUNT);
    const bool ran = sched->run_on_loop([&] {
        // between flights: what the stepping thread owns of an idle session does not move.  A session that was fed or closed meanwhile, or
        // whose flush has not finished, is refused.
        std::vector<SnapRec> recs; std::vector<uint8_t *> dst; std::vector<int> who;
        for (int i = 0; i < n; ++i) {
            Session &s = *ss[i];
            if (ok[i]) ok[i] = !s.closing && s.submitted == s.completed && !s.busy && !s.fed && !s.flush_requested && s.flush_phase == 0 && s.queued() == 0 && !s.borrow_cnt && !s.fb.lent() &&
                               s.fb.avail >= 0 && s.fb.avail <= s.fb.ring_frames;
            if (!ok[i]) continue;
            SnapRec r;
            r.slot = s.slot; r.tail = s.fb.tail; r.rows = (int32_t)s.fb.avail; r.tgt_tail = 0; r.mask = device_mask(s);
            std::vector<uint8_t> &dev = blocks[(size_t)i * snap::B_COUNT + snap::B_DEVICE];
            const uint32_t bytes = lay.block_bytes(r.rows);
            snap::Out h;
            h.put<uint32_t>(Engine::SNAP_ARRAYS); h.put<uint32_t>((uint32_t)r.rows); h.put<uint32_t>(r.mask); h.put<uint32_t>(bytes);
            for (int a = 0; a < Engine::SNAP_ARRAYS; ++a) { h.put(lay.arr[a].layers); h.put(lay.arr[a].row_bytes); h.put(lay.arr[a].off); h.put<uint32_t>(0); }
            dev = std::move(h.b);
            dev.resize(kDeviceHeader + bytes);
            recs.push_back(r); dst.push_back(dev.data() + kDeviceHeader); who.push_back(i);
            // the host's share, while nothing moves
            snap::Out g, b, q, f;
            snap::write_greedy(snap::Access::capture(s.greedy), g); snap::write_book(snap::capture_book(s.fb), b); snap::write_session(snap::capture_session(s), q);
            const AprilxSnapshotInfo info = snapshot_info_of(s);
            f.bytes(&info, sizeof info);
            blocks[(size_t)i * snap::B_COUNT + snap::B_INFO] = std::move(f.b); blocks[(size_t)i * snap::B_COUNT + snap::B_GREEDY] = std::move(g.b);
            blocks[(size_t)i * snap::B_COUNT + snap::B_BOOK] = std::move(b.b); blocks[(size_t)i * snap::B_COUNT + snap::B_SESSION] = std::move(q.b);
        }
        // (a caller that only asks for the sizes gets blobs of the right length whose device blocks are zeros: nothing is launched)
        if (!sizes_only && !recs.empty() && !eng->snapshot_gather((int)recs.size(), recs.data(), dst.data())) for (int i : who) ok[i] = false;
    });
    for (int i = 0; i < n; ++i) {
        if (!ran) ok[i] = false;
        if (!ok[i]) continue;
        std::vector<uint8_t> five[snap::B_COUNT];
        for (int k = 0; k < snap::B_COUNT; ++k) five[k] = std::move(blocks[(size_t)i * snap::B_COUNT + k]);
        out[i] = snap::assemble(five);
        // (the total size is part of the info block: written once the blob exists, then the hash again)
        AprilxSnapshotInfo *info = reinterpret_cast<AprilxSnapshotInfo *>(out[i].data() + snap::kHeaderBytes);
        const uint64_t total = out[i].size();
        memcpy(&info->blob_size, &total, 8);
        const uint64_t h = snap::fnv1a(out[i].data(), out[i].size() - 8);
        memcpy(out[i].data() + out[i].size() - 8, &h, 8);
    }
}

void snapshot_sessions(size_t n, Session *const *ss, std::vector<uint8_t> *out, bool *ok, bool sizes_only)
{
    std::map<Scheduler *, std::vector<size_t>> groups;
    for (size_t i = 0; i < n; ++i) groups[ss[i]->sched].push_back(i);
    for (auto &g : groups) {
        const int m = (int)g.second.size();
        std::vector<Session *> sub((size_t)m); std::vector<std::vector<uint8_t>> blobs((size_t)m); std::unique_ptr<bool[]> good(new bool[(size_t)m]);
        for (int k = 0; k < m; ++k) sub[(size_t)k] = ss[g.second[(size_t)k]];
        snapshot_group(g.first, sub.data(), m, blobs.data(), good.get(), sizes_only);
        for (int k = 0; k < m; ++k) { ok[g.second[(size_t)k]] = good[(size_t)k]; out[g.second[(size_t)k]] = std::move(blobs[(size_t)k]); }
    }
}

// ---------------------------------------------------------------- restore
namespace {
struct Parsed {
    snap::GreedyImage greedy; snap::BookImage book; snap::SessionImage sess; AprilxSnapshotInfo info;
    const uint8_t *device = nullptr; uint32_t rows = 0, mask = 0;
};

// everything that can be decided without the GPU: the blob parses, every value is in range, model, precision and configuration agree
const char *parse_for(const Session &s, const Engine::SnapLayout &lay, const void *blob, size_t size, Parsed *p)
{
    snap::View v;
    const char *why = "corrupt blob";
    if (!snap::parse(blob, size, &v, &why)) return why;
    memcpy(&p->info, v.blk[snap::B_INFO], sizeof p->info);
    if (p->info.blob_size != (uint64_t)size) return "info block: size differs";
    const AprilxSnapshotInfo mine = snapshot_info_of(s);
    if (const char *m = snapshot_mismatch(p->info, mine)) return m;
    snap::In g(v.blk[snap::B_GREEDY], v.len[snap::B_GREEDY]), b(v.blk[snap::B_BOOK], v.len[snap::B_BOOK]), q(v.blk[snap::B_SESSION], v.len[snap::B_SESSION]);
    if (!snap::read_greedy(g, mine.vocab, s.greedy.bias() ? s.greedy.bias()->states() : 0, &p->greedy, &why)) return why;
    if (!snap::read_book(b, &p->book, &why)) return why;
    if (!snap::read_session(q, &p->sess, &why)) return why;
    // the images against the configuration they were checked with
    const snap::BookImage &k = p->book;
    const FrameBook &fb = s.fb;
    if (k.shift != fb.shift || k.padded != fb.padded || k.seg_count != fb.seg_count || k.seg_step != fb.seg_step) return "frame geometry differs";
    if ((k.rs_in_rate != 0) != (fb.rs != nullptr) || (fb.rs && (k.rs_in_rate != fb.rs->in_rate || k.rs_out_rate != fb.rs->out_rate))) return "frame book: input rate differs";
    if (!same(k.fmt, fb.fmt)) return "frame book: input format differs";
    if (k.avail > fb.ring_frames) return "more ring rows than the target's ring holds";
    if (p->greedy.conf_k != (uint32_t)s.greedy.confidence()) return "search state: confidence alternatives differ";
    if (!s.greedy.bias() && p->greedy.bias_state != 0) return "trie state without a set";
    if ((p->sess.vad_on != 0) != s.vad.on || (p->sess.dtmf_on != 0) != s.dtmf.on || (p->sess.tones_on != 0) != s.tones.on) return "detector state differs from the configuration";
    if (p->sess.real_frames != p->info.frames_seen || p->sess.chunks != p->info.chunks || k.rows_written != p->info.rows_written) return "counters disagree";
    // the device block: the layout must be this engine's
    snap::In d(v.blk[snap::B_DEVICE], v.len[snap::B_DEVICE]);
    uint32_t na = 0, bytes = 0;
    d.get(na); d.get(p->rows); d.get(p->mask); d.get(bytes);
    if (!d.ok || na != (uint32_t)Engine::SNAP_ARRAYS || (int64_t)p->rows != k.avail || p->rows != p->info.ring_rows) return "device block: header out of range";
    for (int a = 0; a < Engine::SNAP_ARRAYS; ++a) {
        uint32_t l = 0, rb = 0, off = 0, z = 0;
        d.get(l); d.get(rb); d.get(off); d.get(z);
        if (!d.ok || l != lay.arr[a].layers || rb != lay.arr[a].row_bytes || off != lay.arr[a].off || z) return "device block: another layout";
    }
    if (bytes != lay.block_bytes((int)p->rows) || v.len[snap::B_DEVICE] != kDeviceHeader + bytes) return "device block: wrong length";
    if (p->mask != device_mask_of(p->sess, s)) return "device block: state mask differs from the session's";
    p->device = v.blk[snap::B_DEVICE] + kDeviceHeader;
    return nullptr;
}
}  // namespace

// n sessions of ONE scheduler
static void restore_group(Scheduler *sched, Session *const *ss, int n, const void *const *blobs, const size_t *sizes, int *status, std::string *errs)
{
    Engine *eng = sched->engine();
    const Engine::SnapLayout lay = eng->snapshot_layout();
    std::vector<Parsed> parsed((size_t)n);
    auto refuse = [&](int i, const char *why) { status[i] = -1; errs[i] = why; };
    for (int i = 0; i < n; ++i) {
        status[i] = 0;
        if (sched->in_own_handler(ss[i])) { refuse(i, "called from a handler"); continue; }
        for (int j = 0; j < i; ++j) if (ss[j] == ss[i]) refuse(i, "the same session twice in one call");
    }
    if (sched->on_loop_thread()) return;
    sched->wait_idle_many(ss, n);
    for (int i = 0; i < n; ++i) {
        if (status[i]) continue;
        if (!fresh(*ss[i])) { refuse(i, "the target session has been fed (or has work queued): only a fresh session can be restored into"); continue; }
        if (ss[i]->greedy.lm()) { refuse(i, "the target session has a language model: a snapshot does not carry the model's node"); continue; }
        if (ss[i]->quality.on) { refuse(i, "the target session has the line-quality observer on: a snapshot does not carry its machine"); continue; }
        if (const char *why = parse_for(*ss[i], lay, blobs[i], sizes[i], &parsed[(size_t)i])) refuse(i, why);
    }
    const bool ran = sched->run_on_loop([&] {
        std::vector<SnapRec> recs; std::vector<const uint8_t *> src; std::vector<int> who;
        for (int i = 0; i < n; ++i) {
            if (status[i]) continue;
            Session &s = *ss[i];
            if (!fresh(s)) { refuse(i, "the target session was fed during the call"); continue; }
            const Parsed &p = parsed[(size_t)i];
            const int R = s.fb.ring_frames, head = (int)(p.book.rows_written % (uint64_t)R);
            SnapRec r;
            r.slot = s.slot; r.rows = (int32_t)p.rows; r.mask = p.mask; r.tail = 0;
            r.tgt_tail = (int)(((int64_t)head - p.book.avail % R + R) % R);
            recs.push_back(r); src.push_back(p.device); who.push_back(i);
        }
        if (recs.empty()) return;
        if (!eng->snapshot_scatter((int)recs.size(), recs.data(), src.data())) { for (int i : who) refuse(i, "the engine refused the device block"); return; }
        for (int i : who) {
            Session &s = *ss[i];
            const Parsed &p = parsed[(size_t)i];
            snap::Access::apply(p.greedy, s.greedy); snap::apply_book(p.book, s.fb); snap::apply_session(p.sess, s);
        }
    });
    if (!ran) for (int i = 0; i < n; ++i) if (!status[i]) refuse(i, "the scheduler is stopping");
}

void restore_sessions(size_t n, Session *const *ss, const void *const *blobs, const size_t *sizes, int *status, std::string *errs)
{
    std::map<Scheduler *, std::vector<size_t>> groups;
    for (size_t i = 0; i < n; ++i) groups[ss[i]->sched].push_back(i);
    for (auto &g : groups) {
        const int m = (int)g.second.size();
        std::vector<Session *> sub((size_t)m); std::vector<const void *> b((size_t)m); std::vector<size_t> z((size_t)m); std::vector<int> st((size_t)m); std::vector<std::string> er((size_t)m);
        for (int k = 0; k < m; ++k) { const size_t i = g.second[(size_t)k]; sub[(size_t)k] = ss[i]; b[(size_t)k] = blobs[i]; z[(size_t)k] = sizes[i]; }
        restore_group(g.first, sub.data(), m, b.data(), z.data(), st.data(), er.data());
        for (int k = 0; k < m; ++k) { status[g.second[(size_t)k]] = st[(size_t)k]; errs[g.second[(size_t)k]] = std::move(er[(size_t)k]); }
    }
}

}  // namespace aprilx
