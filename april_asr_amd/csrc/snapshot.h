// Session snapshot / restore, the host half (include/aprilx_engine.h "session snapshot and restore"; DESIGN.md section 19 has the
// format byte by byte): pure functions over the fields of Greedy, FrameBook and Session, and the blob's container.  Header-only and
// free of the engine on purpose: tests/cpp/snapshot_test.cc builds it alone under the sanitizers, and the scheduler harness builds
// session.cc without further files.  Everything is little-endian and written field by field (no struct is copied as memory except the
// public POD structs of the ABI, whose layout is pinned).
//
//   capture_*   fields -> an image (plain data)          write_*   image -> bytes
//   read_*      bytes -> image, every value checked      apply_*   image -> fields of a FRESH session (nothing fails from here on)
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "session.h"

namespace aprilx {
namespace snap {

constexpr char kMagic[8] = {'A', 'P', 'X', 'S', 'N', 'A', 'P', '1'};
constexpr uint32_t kVersion = 1;
enum { B_INFO = 0, B_GREEDY = 1, B_BOOK = 2, B_SESSION = 3, B_DEVICE = 4, B_COUNT = 5 };
constexpr size_t kHeaderBytes = 24 + 16 * B_COUNT + 24;      // magic, version, block count, size; (offset, length) per block; 3 reserved words = 128
static_assert(kHeaderBytes == 128, "DESIGN.md section 19");
static_assert(sizeof(AprilxSnapshotInfo) == 512 && sizeof(AprilxTokenInfo) == 96, "the blob carries them as bytes");

inline uint64_t fnv1a(const void *p, size_t n, uint64_t h = 0xcbf29ce484222325ull)
{
    const uint8_t *b = static_cast<const uint8_t *>(p);
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 0x100000001b3ull; }
    return h;
}

struct Out {
    std::vector<uint8_t> b;
    void bytes(const void *p, size_t n) { if (n) { const uint8_t *q = static_cast<const uint8_t *>(p); b.insert(b.end(), q, q + n); } }
    template <typename T> void put(T v) { bytes(&v, sizeof v); }
    void pad(size_t a) { while (b.size() % a) b.push_back(0); }
};
// never reads past n: a failed read leaves ok false and every later one fails too
struct In {
    const uint8_t *p; size_t n; size_t pos = 0; bool ok = true;
    In(const void *data, size_t size) : p(static_cast<const uint8_t *>(data)), n(size) {}
    bool bytes(void *dst, size_t k) { if (!ok || k > n - pos) { ok = false; return false; } if (k) memcpy(dst, p + pos, k); pos += k; return true; }
    template <typename T> bool get(T &v) { return bytes(&v, sizeof v); }
    bool skip_pad(size_t a) { while (ok && pos % a) { uint8_t z; if (!get(z) || z) ok = false; } return ok; }
    bool done() const { return ok && pos == n; }
};

// ---------------------------------------------------------------- the container
struct View { const uint8_t *blk[B_COUNT]; size_t len[B_COUNT]; };
inline void set_why(const char **why, const char *msg) { if (why) *why = msg; }

// magic, version, size, block table (in order, 8-byte aligned, inside [header, size - 8)), trailing hash
inline bool parse(const void *blob, size_t size, View *v, const char **why = nullptr)
{
    if (!blob || size < kHeaderBytes + 8) { set_why(why, "blob shorter than its header"); return false; }
    In in(blob, kHeaderBytes);
    char magic[8]; uint32_t version = 0, nblk = 0; uint64_t total = 0;
    in.bytes(magic, 8); in.get(version); in.get(nblk); in.get(total);
    if (memcmp(magic, kMagic, 8) != 0) { set_why(why, "not a snapshot (magic)"); return false; }
    if (version != kVersion) { set_why(why, "snapshot of another format version"); return false; }
    if (nblk != B_COUNT || total != (uint64_t)size) { set_why(why, "size field differs from the bytes given"); return false; }
    uint64_t at = kHeaderBytes;
    for (int i = 0; i < B_COUNT; ++i) {
        uint64_t off = 0, len = 0;
        in.get(off); in.get(len);
        if (off != at || off % 8 || len > (uint64_t)size - 8 - off) { set_why(why, "block table out of bounds"); return false; }
        v->blk[i] = static_cast<const uint8_t *>(blob) + off; v->len[i] = (size_t)len;
        at = (off + len + 7) / 8 * 8;
    }
    for (int i = 0; i < 3; ++i) { uint64_t z = 1; in.get(z); if (z) { set_why(why, "reserved header words are not zero"); return false; } }
    if (at != (uint64_t)size - 8) { set_why(why, "blocks do not fill the blob"); return false; }
    uint64_t h = 0;
    memcpy(&h, static_cast<const uint8_t *>(blob) + size - 8, 8);
    if (h != fnv1a(blob, size - 8)) { set_why(why, "hash mismatch (corrupt blob)"); return false; }
    if (v->len[B_INFO] != sizeof(AprilxSnapshotInfo)) { set_why(why, "info block of another size"); return false; }
    return true;
}

inline std::vector<uint8_t> assemble(const std::vector<uint8_t> (&blocks)[B_COUNT])
{
    Out o;
    o.bytes(kMagic, 8); o.put<uint32_t>(kVersion); o.put<uint32_t>(B_COUNT);
    uint64_t total = kHeaderBytes;
    for (int i = 0; i < B_COUNT; ++i) total += (blocks[i].size() + 7) / 8 * 8;
    total += 8;
    o.put<uint64_t>(total);
    uint64_t at = kHeaderBytes;
    for (int i = 0; i < B_COUNT; ++i) { o.put<uint64_t>(at); o.put<uint64_t>(blocks[i].size()); at += (blocks[i].size() + 7) / 8 * 8; }
    for (int i = 0; i < 3; ++i) o.put<uint64_t>(0);
    for (int i = 0; i < B_COUNT; ++i) { o.bytes(blocks[i].data(), blocks[i].size()); o.pad(8); }
    o.put<uint64_t>(fnv1a(o.b.data(), o.b.size()));
    return std::move(o.b);
}

// ---------------------------------------------------------------- Greedy
struct GreedyImage {
    int32_t ctx[2] = {0, 0}, bias_state = 0; uint32_t conf_k = 0;
    uint64_t evals = 0, head = 0, last_call_head = 0, last_emit_ms = 0, first_ms = 0;
    uint8_t emitted_silence = 1;
    // the entries of active_[] the state machine can still read: [0, max(head, last_call_head)) -- a provisional token sits AT head
    struct Tok { int32_t id = -1; float logprob = 0; uint32_t flags = 0; uint64_t time_ms = 0; };
    std::vector<Tok> toks;
    std::vector<AprilxTokenInfo> infos;                       // conf_k > 0: one per entry
};

struct Access {      // (friend of Greedy)
    static GreedyImage capture(const Greedy &g)
    {
        GreedyImage m;
        m.ctx[0] = g.ctx[0]; m.ctx[1] = g.ctx[1]; m.bias_state = g.bias_state_; m.conf_k = (uint32_t)g.conf_k_;
        m.evals = g.evals_; m.head = g.head_; m.last_call_head = g.last_call_head_; m.last_emit_ms = g.last_emit_ms_; m.first_ms = g.first_ms_;
        m.emitted_silence = g.emitted_silence_ ? 1 : 0;
        const size_t n = std::min<size_t>(Greedy::kMaxActive, std::max(g.head_, g.last_call_head_));
        for (size_t i = 0; i < n; ++i) {
            GreedyImage::Tok t;
            t.id = g.active_id_[i]; t.logprob = g.active_[i].logprob; t.flags = (uint32_t)g.active_[i].flags; t.time_ms = (uint64_t)g.active_[i].time_ms;
            m.toks.push_back(t);
            if (g.conf_k_) m.infos.push_back(g.info_[i]);
        }
        return m;
    }
    // the token pointers are rebuilt from the ids; the set, K and the options are the target's own (checked equal before)
    static void apply(const GreedyImage &m, Greedy &g)
    {
        g.ctx[0] = m.ctx[0]; g.ctx[1] = m.ctx[1]; g.ctx_dirty = false; g.bias_state_ = m.bias_state;
        g.evals_ = m.evals; g.head_ = (size_t)m.head; g.last_call_head_ = (size_t)m.last_call_head; g.last_emit_ms_ = (size_t)m.last_emit_ms;
        g.first_ms_ = (size_t)m.first_ms; g.emitted_silence_ = m.emitted_silence != 0;
        for (size_t i = 0; i < m.toks.size(); ++i) {
            const GreedyImage::Tok &t = m.toks[i];
            AprilToken &a = g.active_[i];
            a.token = t.id >= 0 ? g.P_->token((size_t)t.id) : nullptr; a.logprob = t.logprob; a.flags = (AprilTokenFlagBits)t.flags; a.time_ms = (size_t)t.time_ms; a.reserved = nullptr;
            g.active_id_[i] = t.id;
            if (g.conf_k_ && i < m.infos.size()) g.info_[i] = m.infos[i];
        }
    }
};

inline void write_greedy(const GreedyImage &m, Out &o)
{
    o.put(m.ctx[0]); o.put(m.ctx[1]); o.put(m.bias_state); o.put(m.conf_k);
    o.put(m.evals); o.put(m.head); o.put(m.last_call_head); o.put(m.last_emit_ms); o.put(m.first_ms);
    o.put<uint32_t>(m.emitted_silence); o.put<uint32_t>((uint32_t)m.toks.size());
    for (const GreedyImage::Tok &t : m.toks) { o.put(t.id); o.put(t.logprob); o.put(t.flags); o.put<uint32_t>(0); o.put(t.time_ms); }
    for (const AprilxTokenInfo &i : m.infos) o.bytes(&i, sizeof i);
}

// vocab, bias_states: the target's (ids and the trie state are indices there)
inline bool read_greedy(In &in, int vocab, int bias_states, GreedyImage *m, const char **why = nullptr)
{
    uint32_t sil = 0, n = 0;
    in.get(m->ctx[0]); in.get(m->ctx[1]); in.get(m->bias_state); in.get(m->conf_k);
    in.get(m->evals); in.get(m->head); in.get(m->last_call_head); in.get(m->last_emit_ms); in.get(m->first_ms);
    in.get(sil); in.get(n);
    if (!in.ok || sil > 1 || n > (uint32_t)Greedy::kMaxActive || m->head >= (uint64_t)Greedy::kMaxActive || m->last_call_head > (uint64_t)Greedy::kMaxActive ||
        (uint64_t)n != std::min<uint64_t>(Greedy::kMaxActive, std::max(m->head, m->last_call_head)) || m->conf_k > 8u) { set_why(why, "search state out of range"); return false; }
    auto tok_ok = [&](int32_t t) { return t >= 0 && t < vocab; };
    if (!(tok_ok(m->ctx[0]) && tok_ok(m->ctx[1])) && !(m->ctx[0] == 0 && m->ctx[1] == 0)) { set_why(why, "context token out of range"); return false; }
    if (m->bias_state < 0 || m->bias_state >= std::max(1, bias_states)) { set_why(why, "trie state out of range"); return false; }
    m->emitted_silence = (uint8_t)sil;
    m->toks.resize(n);
    for (GreedyImage::Tok &t : m->toks) {
        uint32_t z = 0;
        in.get(t.id); in.get(t.logprob); in.get(t.flags); in.get(z); in.get(t.time_ms);
        if (!in.ok || z || t.id < -1 || t.id >= vocab) { set_why(why, "active token out of range"); return false; }
    }
    for (uint64_t i = 0; i < m->head; ++i) if (m->toks[(size_t)i].id < 0) { set_why(why, "active token without an id"); return false; }
    if (m->conf_k) { m->infos.resize(n); for (AprilxTokenInfo &i : m->infos) in.bytes(&i, sizeof i); }
    if (!in.done()) { set_why(why, "search block of the wrong length"); return false; }
    return true;
}

// ---------------------------------------------------------------- FrameBook
struct BookImage {
    int32_t shift = 0, padded = 0, seg_count = 0, seg_step = 0, ring_frames = 0, head = 0, tail = 0;
    int64_t avail = 0, avail_shadow = 0; uint64_t rows_written = 0, fifo_pos = 0; int64_t in_drop = 0, rs_end = 0;
    uint32_t rs_in_rate = 0, rs_out_rate = 0;                 // 0, 0: not resampled
    InputFormat fmt;
    std::vector<FrameBook::RsSeg> segs;
    std::vector<uint8_t> audio;                               // the unconsumed queue: int16 samples (little-endian), or the raw bytes of a formatted session
};

// an idle session: nothing is lent.  Plain sessions leave the consumed samples behind (fifo_pos becomes 0: the positions are relative to
// the fifo there); segmented ones keep their queue as it is (its positions are absolute, in_drop says where it starts).
inline BookImage capture_book(const FrameBook &fb)
{
    BookImage m;
    m.shift = fb.shift; m.padded = fb.padded; m.seg_count = fb.seg_count; m.seg_step = fb.seg_step; m.ring_frames = fb.ring_frames; m.head = fb.head; m.tail = fb.tail;
    m.avail = fb.avail; m.avail_shadow = fb.avail_shadow; m.rows_written = fb.rows_written; m.fifo_pos = fb.fifo_pos; m.in_drop = fb.in_drop; m.rs_end = fb.rs_end;
    if (fb.rs) { m.rs_in_rate = fb.rs->in_rate; m.rs_out_rate = fb.rs->out_rate; }
    m.fmt = fb.fmt;
    m.segs.assign(fb.segs.begin(), fb.segs.end());
    if (fb.fmt) m.audio = fb.raw.bytes;
    else {
        const size_t skip = fb.segmented() ? 0 : std::min(fb.fifo_pos, fb.fifo.size());
        if (!fb.segmented()) m.fifo_pos = fb.fifo_pos - skip;
        m.audio.resize((fb.fifo.size() - skip) * 2);
        for (size_t i = skip; i < fb.fifo.size(); ++i) { const uint16_t v = (uint16_t)fb.fifo[i]; m.audio[(i - skip) * 2] = (uint8_t)(v & 0xff); m.audio[(i - skip) * 2 + 1] = (uint8_t)(v >> 8); }
    }
    return m;
}

inline void write_book(const BookImage &m, Out &o)
{
    o.put(m.shift); o.put(m.padded); o.put(m.seg_count); o.put(m.seg_step); o.put(m.ring_frames); o.put(m.head); o.put(m.tail); o.put<uint32_t>(0);
    o.put(m.avail); o.put(m.avail_shadow); o.put(m.rows_written); o.put(m.fifo_pos); o.put(m.in_drop); o.put(m.rs_end);
    o.put(m.rs_in_rate); o.put(m.rs_out_rate); o.put(m.fmt.encoding); o.put(m.fmt.channels); o.put(m.fmt.channel); o.put(m.fmt.frame_bytes);
    o.put<uint32_t>((uint32_t)m.segs.size()); o.put<uint32_t>(0); o.put<uint64_t>(m.audio.size());
    for (const FrameBook::RsSeg &s : m.segs) { o.put(s.pos); o.put(s.in_start); o.put(s.n_in); o.put(s.n_out); o.put(s.zeros); o.put<uint64_t>(s.closed ? 1 : 0); }
    o.bytes(m.audio.data(), m.audio.size());
}

inline bool read_book(In &in, BookImage *m, const char **why = nullptr)
{
    uint32_t z0 = 0, z1 = 0, nseg = 0; uint64_t abytes = 0;
    in.get(m->shift); in.get(m->padded); in.get(m->seg_count); in.get(m->seg_step); in.get(m->ring_frames); in.get(m->head); in.get(m->tail); in.get(z0);
    in.get(m->avail); in.get(m->avail_shadow); in.get(m->rows_written); in.get(m->fifo_pos); in.get(m->in_drop); in.get(m->rs_end);
    in.get(m->rs_in_rate); in.get(m->rs_out_rate); in.get(m->fmt.encoding); in.get(m->fmt.channels); in.get(m->fmt.channel); in.get(m->fmt.frame_bytes);
    in.get(nseg); in.get(z1); in.get(abytes);
    if (!in.ok || z0 || z1) { set_why(why, "frame book truncated"); return false; }
    if (m->shift <= 0 || m->padded <= 0 || m->seg_count <= 0 || m->seg_step <= 0 || m->ring_frames < m->seg_count || m->head < 0 || m->head >= m->ring_frames ||
        m->tail < 0 || m->tail >= m->ring_frames || m->avail < 0 || m->avail > m->ring_frames || m->avail_shadow > m->avail || m->avail_shadow < -(int64_t)m->ring_frames ||
        (uint64_t)m->head != m->rows_written % (uint64_t)m->ring_frames || (m->tail + m->avail) % m->ring_frames != m->head || m->in_drop < 0 || m->rs_end < 0 ||
        m->fifo_pos > ((uint64_t)1 << 62)) { set_why(why, "frame book out of range"); return false; }
    if (m->fmt.frame_bytes && (!input_format_valid(m->fmt.encoding, m->fmt.channels, m->fmt.channel) || m->fmt.frame_bytes != encoding_bytes(m->fmt.encoding) * m->fmt.channels)) {
        set_why(why, "input format out of range"); return false;
    }
    const bool segmented = m->rs_in_rate != 0 || m->fmt.frame_bytes != 0;
    if (nseg > 64 || (segmented && nseg == 0) || (!segmented && nseg != 0) || abytes > in.n - in.pos || abytes % (m->fmt.frame_bytes ? m->fmt.frame_bytes : 2u)) {
        set_why(why, "audio queue out of range"); return false;
    }
    m->segs.resize(nseg);
    for (FrameBook::RsSeg &s : m->segs) {
        uint64_t c = 0;
        in.get(s.pos); in.get(s.in_start); in.get(s.n_in); in.get(s.n_out); in.get(s.zeros); in.get(c);
        if (!in.ok || c > 1 || s.pos < 0 || s.in_start < 0 || s.n_in < 0 || s.n_out < 0 || s.zeros < 0) { set_why(why, "segment out of range"); return false; }
        s.closed = c != 0;
    }
    for (size_t i = 1; i < m->segs.size(); ++i) if (m->segs[i].pos < m->segs[i - 1].pos || m->segs[i].in_start < m->segs[i - 1].in_start) { set_why(why, "segments out of order"); return false; }
    if (segmented && (m->segs.front().pos > (int64_t)m->fifo_pos || m->segs.back().in_start + m->segs.back().n_in != m->in_drop + (int64_t)(abytes / (m->fmt.frame_bytes ? m->fmt.frame_bytes : 2u)))) {
        set_why(why, "segments do not match the audio queue"); return false;
    }
    if (!segmented && m->fifo_pos > abytes / 2) { set_why(why, "audio queue shorter than its position"); return false; }
    m->audio.resize((size_t)abytes);
    in.bytes(m->audio.data(), (size_t)abytes);
    if (!in.done()) { set_why(why, "frame book of the wrong length"); return false; }
    return true;
}

// Ring positions are re-based: the target's ring may have another length.  head stays rows_written % ring_frames (what
// aprilx_session_read_frames indexes with), the tail follows from avail; the frame clock and rows_written continue.  `fb` is the fresh
// target's book: geometry, rs and fmt are its own (checked equal before).
inline void apply_book(const BookImage &m, FrameBook &fb)
{
    fb.rows_written = m.rows_written; fb.avail = (long)m.avail; fb.avail_shadow = (long)m.avail_shadow;
    fb.head = (int)(m.rows_written % (uint64_t)fb.ring_frames);
    fb.tail = (int)(((int64_t)fb.head - m.avail % fb.ring_frames + fb.ring_frames) % fb.ring_frames);
    fb.fifo_pos = (size_t)m.fifo_pos; fb.in_drop = m.in_drop; fb.rs_end = m.rs_end;
    fb.ext = nullptr; fb.ext_cnt = 0;
    fb.segs.assign(m.segs.begin(), m.segs.end());
    fb.fifo.clear(); fb.raw.clear();
    if (fb.fmt) { fb.raw.fbytes = fb.fmt.frame_bytes; fb.raw.bytes = m.audio; }
    else {
        fb.fifo.resize(m.audio.size() / 2);
        for (size_t i = 0; i < fb.fifo.size(); ++i) fb.fifo[i] = (int16_t)((uint16_t)m.audio[2 * i] | (uint16_t)((uint16_t)m.audio[2 * i + 1] << 8));
    }
}

// ---------------------------------------------------------------- Session (its own fields and the detectors' machines and counters)
struct SessionImage {
    uint8_t dout_ready = 0, was_flushed = 0, seg_open = 0, vad_on = 0, vad_reset = 1, dtmf_on = 0, tones_on = 0;
    uint64_t now_ms = 0, chunks = 0, real_frames = 0;
    uint64_t vad_speech = 0; uint32_t vad_segments = 0; int32_t vad_last = 0;
    DtmfMachine dm; uint64_t dtmf_tone = 0, dtmf_digits = 0;
    ToneMachine tm; uint64_t tonal = 0, tones = 0;
};

inline SessionImage capture_session(const Session &s)
{
    SessionImage m;
    m.dout_ready = s.dout_ready; m.was_flushed = s.was_flushed; m.seg_open = s.seg_open;
    m.vad_on = s.vad.on; m.vad_reset = s.vad.reset; m.dtmf_on = s.dtmf.on; m.tones_on = s.tones.on;
    m.now_ms = s.now_ms; m.chunks = s.chunks; m.real_frames = s.real_frames;
    m.vad_speech = s.vad.speech; m.vad_segments = s.vad.segments; m.vad_last = s.vad.last;
    m.dm = s.dtmf.m; m.dtmf_tone = s.dtmf.tone; m.dtmf_digits = s.dtmf.digits;
    m.tm = s.tones.m; m.tonal = s.tones.tonal; m.tones = s.tones.tones;
    return m;
}

inline void write_session(const SessionImage &m, Out &o)
{
    const uint8_t f[8] = {m.dout_ready, m.was_flushed, m.seg_open, m.vad_on, m.vad_reset, m.dtmf_on, m.tones_on, 0};
    o.bytes(f, 8);
    o.put(m.now_ms); o.put(m.chunks); o.put(m.real_frames);
    o.put(m.vad_speech); o.put(m.vad_segments); o.put(m.vad_last);
    o.put(m.dm.held); o.put(m.dm.cand); o.put(m.dm.run); o.put<uint32_t>(0); o.put(m.dtmf_tone); o.put(m.dtmf_digits);
    o.put(m.tm.held); o.put(m.tm.h1); o.put(m.tm.h2); o.put(m.tm.c1); o.put(m.tm.c2); o.put(m.tm.run); o.put(m.tonal); o.put(m.tones);
}

inline bool read_session(In &in, SessionImage *m, const char **why = nullptr)
{
    uint8_t f[8]; uint32_t z = 0;
    in.bytes(f, 8);
    in.get(m->now_ms); in.get(m->chunks); in.get(m->real_frames);
    in.get(m->vad_speech); in.get(m->vad_segments); in.get(m->vad_last);
    in.get(m->dm.held); in.get(m->dm.cand); in.get(m->dm.run); in.get(z); in.get(m->dtmf_tone); in.get(m->dtmf_digits);
    in.get(m->tm.held); in.get(m->tm.h1); in.get(m->tm.h2); in.get(m->tm.c1); in.get(m->tm.c2); in.get(m->tm.run); in.get(m->tonal); in.get(m->tones);
    if (!in.done() || z || f[7]) { set_why(why, "session block of the wrong length"); return false; }
    for (int i = 0; i < 7; ++i) if (f[i] > 1) { set_why(why, "session flag out of range"); return false; }
    auto hz = [](int32_t v) { return v >= 0 && v <= 65535; };
    if (m->vad_last < 0 || m->vad_last > 1 || m->dm.held < 0 || m->dm.held > 16 || m->dm.cand < 0 || m->dm.cand > 16 || m->dm.run < 0 || m->tm.held < 0 || m->tm.held > 1 ||
        !hz(m->tm.h1) || !hz(m->tm.h2) || !hz(m->tm.c1) || !hz(m->tm.c2) || m->tm.run < 0) { set_why(why, "detector state out of range"); return false; }
    m->dout_ready = f[0]; m->was_flushed = f[1]; m->seg_open = f[2]; m->vad_on = f[3]; m->vad_reset = f[4]; m->dtmf_on = f[5]; m->tones_on = f[6];
    return true;
}

// the options, plans and handlers are the target's own (checked equal before)
inline void apply_session(const SessionImage &m, Session &s)
{
    s.dout_ready = m.dout_ready; s.was_flushed = m.was_flushed; s.seg_open = m.seg_open;
    s.now_ms = (size_t)m.now_ms; s.chunks = m.chunks; s.real_frames = m.real_frames;
    s.vad.reset = m.vad_reset; s.vad.speech = m.vad_speech; s.vad.segments = m.vad_segments; s.vad.last = m.vad_last;
    s.dtmf.m = m.dm; s.dtmf.tone = m.dtmf_tone; s.dtmf.digits = m.dtmf_digits;
    s.tones.m = m.tm; s.tones.tonal = m.tonal; s.tones.tones = m.tones;
}

}  // namespace snap
}  // namespace aprilx
