// csrc/snapshot.h alone: the search state machine, the frame book (plain, resampled, formatted with a raw tail)
// and the detectors' machines go through capture -> bytes -> read -> apply and come back field by field; a restored state machine then
// takes the same decisions as the one that went on; the container refuses truncated, flipped and mislabelled blobs.  Built with
// session.cc (the state machine itself) and the scheduler harness's engine, under AddressSanitizer + UBSan.
#include <cstdio>
#include <cstdlib>
#include <random>
#include "snapshot.h"

namespace aprilx { int g_loglevel = 0; }
using namespace aprilx;

static int failures = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static ModelParams make_params()
{
    ModelParams p;
    const char *toks[] = {"<b>", " a", "b", ".", " c", ",", "1", " d", "e", "?", " f", "g"};
    p.token_count = 12; p.blank_id = 0; p.token_stride = 8;
    p.tokens.assign((size_t)p.token_count * p.token_stride, 0);
    for (int i = 0; i < p.token_count; ++i) strcpy(p.tokens.data() + p.token_stride * (size_t)i, toks[i]);
    p.segment_size = 9; p.segment_step = 4; p.frame_shift_ms = 10; p.sample_rate = 16000;
    return p;
}

static bool same_tok(const snap::GreedyImage::Tok &a, const snap::GreedyImage::Tok &b)
{
    return a.id == b.id && memcmp(&a.logprob, &b.logprob, 4) == 0 && a.flags == b.flags && a.time_ms == b.time_ms;
}
static bool same_image(const snap::GreedyImage &a, const snap::GreedyImage &b)
{
    if (a.ctx[0] != b.ctx[0] || a.ctx[1] != b.ctx[1] || a.bias_state != b.bias_state || a.conf_k != b.conf_k || a.evals != b.evals || a.head != b.head ||
        a.last_call_head != b.last_call_head || a.last_emit_ms != b.last_emit_ms || a.first_ms != b.first_ms || a.emitted_silence != b.emitted_silence ||
        a.toks.size() != b.toks.size() || a.infos.size() != b.infos.size()) return false;
    for (size_t i = 0; i < a.toks.size(); ++i) if (!same_tok(a.toks[i], b.toks[i])) return false;
    for (size_t i = 0; i < a.infos.size(); ++i) if (memcmp(&a.infos[i], &b.infos[i], sizeof(AprilxTokenInfo)) != 0) return false;
    return true;
}
static bool same_events(const std::vector<Event> &a, const std::vector<Event> &b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) {
        if (a[i].type != b[i].type || a[i].tokens.size() != b[i].tokens.size() || a[i].infos.size() != b[i].infos.size()) return false;
        for (size_t k = 0; k < a[i].tokens.size(); ++k) {
            const AprilToken &x = a[i].tokens[k], &y = b[i].tokens[k];
            if (x.token != y.token || memcmp(&x.logprob, &y.logprob, 4) != 0 || x.flags != y.flags || x.time_ms != y.time_ms) return false;
        }
        for (size_t k = 0; k < a[i].infos.size(); ++k) if (memcmp(&a[i].infos[k], &b[i].infos[k], sizeof(AprilxTokenInfo)) != 0) return false;
    }
    return true;
}

// a seeded run of joiner results: tokens, blanks, close calls (the provisional-token branch), long silences (the endpoint)
struct Feed {
    std::mt19937 rng; size_t now = 0; ConfRecord side;
    explicit Feed(unsigned seed) : rng(seed) {}
    bool step(Greedy &g, std::vector<Event> &out, bool conf)
    {
        const unsigned r = rng();
        JointResult j;
        j.idx = 1 + (int)(r % 11); j.max_val = (float)((r >> 8) % 1000) / 100.0f; j.blank_val = (float)((r >> 20) % 1000) / 100.0f;
        now += (r >> 4) % 64 == 0 ? 2400 : 40;
        if (conf) {
            memset(&side, 0, sizeof side);
            side.n_alt = 3; side.lse = j.max_val + 1.0f; side.blank_val = j.blank_val;
            for (int i = 0; i < 3; ++i) { side.alt_id[i] = (j.idx + i) % 12; side.alt_logit[i] = j.max_val - (float)i; }
            g.set_side(&side);
        }
        const bool blank = g.on_joint(j, (r >> 30) & 1 ? 1.0f : 0.0f, now, out);
        g.ctx_dirty = false;
        return blank;
    }
};

static void test_greedy(const ModelParams &p, const std::vector<uint8_t> &cls, int conf_k, unsigned seed)
{
    Greedy a;
    a.init(&p, &cls); a.set_confidence(conf_k); a.reset_context_to_blank(); a.ctx_dirty = false;
    Feed fa(seed);
    std::vector<Event> ev;
    int with_active = 0, with_provisional = 0;
    for (int round = 0; round < 400; ++round) {
        fa.step(a, ev, conf_k > 0);
        ev.clear();
        if (round % 7) continue;
        const snap::GreedyImage img = snap::Access::capture(a);
        with_active += img.head > 0; with_provisional += img.last_call_head == img.head + 1;
        snap::Out o;
        snap::write_greedy(img, o);
        snap::In in(o.b.data(), o.b.size());
        snap::GreedyImage back;
        const char *why = nullptr;
        CHECK(snap::read_greedy(in, p.token_count, 0, &back, &why));
        CHECK(same_image(img, back));
        Greedy b;
        b.init(&p, &cls); b.set_confidence(conf_k);
        snap::Access::apply(back, b);
        CHECK(same_image(img, snap::Access::capture(b)));
        // the copy goes on as the source does
        Feed fb = fa; Greedy a2 = a;
        std::vector<Event> ea, eb;
        for (int k = 0; k < 60; ++k) { Feed f2 = fb; const bool x = fb.step(a2, ea, conf_k > 0), y = f2.step(b, eb, conf_k > 0); CHECK(x == y); }
        a2.finish_flush(ea); b.finish_flush(eb);
        CHECK(same_events(ea, eb));
        CHECK(same_image(snap::Access::capture(a2), snap::Access::capture(b)));
        // every truncation of the block is refused; so are values out of range
        for (size_t n = 0; n < o.b.size(); ++n) { snap::In t(o.b.data(), n); snap::GreedyImage x; CHECK(!snap::read_greedy(t, p.token_count, 0, &x)); }
        { snap::In t(o.b.data(), o.b.size()); snap::GreedyImage x; CHECK(img.toks.empty() || !snap::read_greedy(t, 1, 0, &x)); }      // ids beyond a smaller vocabulary
        std::vector<uint8_t> bad = o.b;
        bad[24] = 72;                                                 // head = 72
        { snap::In t(bad.data(), bad.size()); snap::GreedyImage x; CHECK(!snap::read_greedy(t, p.token_count, 0, &x)); }
        bad = o.b; bad[8] = 1;                                        // a trie state without a set
        { snap::In t(bad.data(), bad.size()); snap::GreedyImage x; CHECK(!snap::read_greedy(t, p.token_count, 0, &x)); }
    }
    CHECK(with_active > 5);
    CHECK(with_provisional > 0);
}

static bool same_book(const snap::BookImage &a, const snap::BookImage &b)
{
    if (a.shift != b.shift || a.padded != b.padded || a.seg_count != b.seg_count || a.seg_step != b.seg_step || a.ring_frames != b.ring_frames || a.head != b.head ||
        a.tail != b.tail || a.avail != b.avail || a.avail_shadow != b.avail_shadow || a.rows_written != b.rows_written || a.fifo_pos != b.fifo_pos || a.in_drop != b.in_drop ||
        a.rs_end != b.rs_end || a.rs_in_rate != b.rs_in_rate || a.rs_out_rate != b.rs_out_rate || memcmp(&a.fmt, &b.fmt, sizeof a.fmt) != 0 || a.audio != b.audio ||
        a.segs.size() != b.segs.size()) return false;
    for (size_t i = 0; i < a.segs.size(); ++i) {
        const FrameBook::RsSeg &x = a.segs[i], &y = b.segs[i];
        if (x.pos != y.pos || x.in_start != y.in_start || x.n_in != y.n_in || x.n_out != y.n_out || x.zeros != y.zeros || x.closed != y.closed) return false;
    }
    return true;
}

static FrameBook base_book(int ring, uint64_t rows_written, long avail)
{
    FrameBook fb;
    fb.shift = 160; fb.padded = 512; fb.seg_count = 9; fb.seg_step = 4; fb.ring_frames = ring;
    fb.rows_written = rows_written; fb.head = (int)(rows_written % (uint64_t)ring); fb.avail = avail; fb.avail_shadow = avail - 3;
    fb.tail = (int)(((long)fb.head - avail % ring + ring) % ring);
    return fb;
}

// capture -> bytes -> read -> apply into a fresh book with another ring length -> capture: equal but for the re-based ring positions
static void round_trip_book(const FrameBook &src, FrameBook target, int target_ring)
{
    const snap::BookImage img = snap::capture_book(src);
    snap::Out o;
    snap::write_book(img, o);
    snap::In in(o.b.data(), o.b.size());
    snap::BookImage back;
    const char *why = "";
    CHECK(snap::read_book(in, &back, &why));
    CHECK(same_book(img, back));
    target.shift = src.shift; target.padded = src.padded; target.seg_count = src.seg_count; target.seg_step = src.seg_step; target.ring_frames = target_ring;
    snap::apply_book(back, target);
    snap::BookImage again = snap::capture_book(target);
    CHECK(again.ring_frames == target_ring && again.head == (int)(src.rows_written % (uint64_t)target_ring));
    CHECK((again.tail + again.avail) % target_ring == again.head);
    again.ring_frames = img.ring_frames; again.head = img.head; again.tail = img.tail;
    CHECK(same_book(img, again));
    CHECK(target.stream_end() - target.fifo_pos == src.stream_end() - src.fifo_pos && target.held() <= src.held() && target.can_cut() == src.can_cut());
    for (size_t n = 0; n < o.b.size(); ++n) { snap::In t(o.b.data(), n); snap::BookImage x; CHECK(!snap::read_book(t, &x)); }
    std::vector<uint8_t> bad = o.b;
    bad[24] = 0xff; bad[25] = 0xff; bad[26] = 0xff; bad[27] = 0x7f;      // tail far outside the ring
    { snap::In t(bad.data(), bad.size()); snap::BookImage x; CHECK(!snap::read_book(t, &x)); }
}

static void test_books()
{
    std::mt19937 rng(5);
    {   // plain: consumed samples in front of the position, a tail behind it; the ring has wrapped
        FrameBook fb = base_book(288, 1000, 5);
        fb.fifo.resize(480 + 197);
        for (auto &v : fb.fifo) v = (int16_t)rng();
        fb.fifo_pos = 480;
        const snap::BookImage img = snap::capture_book(fb);
        CHECK(img.fifo_pos == 0 && img.audio.size() == 2 * 197);      // only what framing has not consumed
        round_trip_book(fb, FrameBook(), 8192);
        round_trip_book(fb, FrameBook(), 288);
    }
    {   // never fed
        round_trip_book(base_book(8192, 0, 0), FrameBook(), 288);
    }
    ResampleSpec rs;
    rs.in_rate = 8000; rs.out_rate = 16000; rs.L = 2; rs.M = 1; rs.K = 32;
    {   // resampled, cut inside the second segment: the queue holds input-rate samples from in_drop on
        FrameBook fb = base_book(8192, 350, 2), target;
        fb.rs = &rs; target.rs = &rs;
        FrameBook::RsSeg a, b;
        a.pos = 0; a.in_start = 0; a.n_in = 20000; a.n_out = 40000; a.zeros = 6400; a.closed = true;
        b.pos = 46400; b.in_start = 20000; b.n_in = 5000; b.n_out = resample_avail(5000, 2, 1, 32);
        fb.segs.push_back(a); fb.segs.push_back(b);
        fb.in_drop = 24000; fb.fifo.resize(1000);
        for (auto &v : fb.fifo) v = (int16_t)rng();
        fb.fifo_pos = 55000; fb.rs_end = b.pos + b.n_out;
        round_trip_book(fb, target, 288);
    }
    {   // formatted (2-channel mu-law) with a raw tail, no resampler
        FrameBook fb = base_book(288, 77, 8), target;
        fb.fmt.encoding = ENC_MULAW; fb.fmt.channels = 2; fb.fmt.channel = -1; fb.fmt.frame_bytes = 2; target.fmt = fb.fmt;
        fb.raw.fbytes = 2; fb.raw.bytes.resize(2 * 137);
        for (auto &v : fb.raw.bytes) v = (uint8_t)rng();
        FrameBook::RsSeg a;
        a.pos = 0; a.in_start = 0; a.n_in = 12457; a.n_out = 12457;
        fb.segs.push_back(a);
        fb.in_drop = 12320; fb.fifo_pos = 12320; fb.rs_end = 12457;
        round_trip_book(fb, target, 8192);
        CHECK(snap::capture_book(fb).audio == fb.raw.bytes);
    }
}

static void test_session_block()
{
    std::unique_ptr<Session> s(new Session()), t(new Session());
    s->dout_ready = true; s->was_flushed = false; s->seg_open = true; s->now_ms = 123456; s->chunks = 3086; s->real_frames = 12345;
    s->vad.on = true; s->vad.reset = false; s->vad.speech = 999; s->vad.segments = 7; s->vad.last = 1;
    s->dtmf.on = true; s->dtmf.m.held = 5; s->dtmf.m.cand = 9; s->dtmf.m.run = 2; s->dtmf.tone = 40; s->dtmf.digits = 6;
    s->tones.on = true; s->tones.m.held = 1; s->tones.m.h1 = 480; s->tones.m.h2 = 620; s->tones.m.c1 = 1100; s->tones.m.c2 = 0; s->tones.m.run = 3; s->tones.tonal = 70; s->tones.tones = 2;
    const snap::SessionImage img = snap::capture_session(*s);
    snap::Out o;
    snap::write_session(img, o);
    snap::In in(o.b.data(), o.b.size());
    snap::SessionImage back;
    CHECK(snap::read_session(in, &back));
    t->vad.on = t->dtmf.on = t->tones.on = true;
    snap::apply_session(back, *t);
    CHECK(t->dout_ready && !t->was_flushed && t->seg_open && t->now_ms == 123456 && t->chunks == 3086 && t->real_frames == 12345);
    CHECK(!t->vad.reset && t->vad.speech == 999 && t->vad.segments == 7 && t->vad.last == 1);
    CHECK(t->dtmf.m.held == 5 && t->dtmf.m.cand == 9 && t->dtmf.m.run == 2 && t->dtmf.tone == 40 && t->dtmf.digits == 6);
    CHECK(t->tones.m.held == 1 && t->tones.m.h1 == 480 && t->tones.m.h2 == 620 && t->tones.m.c1 == 1100 && t->tones.m.c2 == 0 && t->tones.m.run == 3 && t->tones.tonal == 70 &&
          t->tones.tones == 2);
    snap::Out again;
    snap::write_session(snap::capture_session(*t), again);
    CHECK(again.b == o.b);
    for (size_t n = 0; n < o.b.size(); ++n) { snap::In x(o.b.data(), n); snap::SessionImage m; CHECK(!snap::read_session(x, &m)); }
    std::vector<uint8_t> bad = o.b;
    bad[0] = 2;                                                       // a flag that is neither 0 nor 1
    { snap::In x(bad.data(), bad.size()); snap::SessionImage m; CHECK(!snap::read_session(x, &m)); }
    bad = o.b; bad[48] = 17;                                          // a DTMF code beyond the 16 digits
    { snap::In x(bad.data(), bad.size()); snap::SessionImage m; CHECK(!snap::read_session(x, &m)); }
}

static void rehash(std::vector<uint8_t> &b) { const uint64_t h = snap::fnv1a(b.data(), b.size() - 8); memcpy(b.data() + b.size() - 8, &h, 8); }

static void test_container()
{
    std::vector<uint8_t> blocks[snap::B_COUNT];
    AprilxSnapshotInfo info;
    memset(&info, 0, sizeof info);
    info.size = sizeof info; info.version = snap::kVersion;
    blocks[snap::B_INFO].assign((const uint8_t *)&info, (const uint8_t *)&info + sizeof info);
    blocks[snap::B_GREEDY].assign(13, 1); blocks[snap::B_BOOK].assign(8, 2); blocks[snap::B_DEVICE].assign(100, 3);
    const std::vector<uint8_t> blob = snap::assemble(blocks);
    snap::View v;
    CHECK(snap::parse(blob.data(), blob.size(), &v));
    CHECK(v.len[snap::B_GREEDY] == 13 && v.len[snap::B_SESSION] == 0 && v.len[snap::B_DEVICE] == 100 && v.blk[snap::B_DEVICE][99] == 3);
    // never past `size`: every truncation is parsed from a heap copy of exactly that length (AddressSanitizer watches the end)
    for (size_t n = 0; n < blob.size(); ++n) { std::vector<uint8_t> cut(blob.begin(), blob.begin() + (long)n); CHECK(!snap::parse(cut.data(), cut.size(), &v)); }
    std::mt19937 rng(19);
    for (int i = 0; i < 200; ++i) {
        std::vector<uint8_t> bad = blob;
        bad[rng() % bad.size()] ^= (uint8_t)(1u << (rng() % 8));
        CHECK(!snap::parse(bad.data(), bad.size(), &v));
    }
    // a wrong magic, version, block count, size and block table, each under a hash that is right
    const size_t at[] = {0, 8, 12, 16, 24, 32, 104};
    for (size_t a : at) { std::vector<uint8_t> bad = blob; bad[a] ^= 1; rehash(bad); CHECK(!snap::parse(bad.data(), bad.size(), &v)); }
    { std::vector<uint8_t> bad = blob; const uint64_t huge = ~0ull; memcpy(bad.data() + 40, &huge, 8); rehash(bad); CHECK(!snap::parse(bad.data(), bad.size(), &v)); }      // a block length that wraps
    { std::vector<uint8_t> same = blob; rehash(same); CHECK(same == blob); }
}

int main()
{
    const ModelParams p = make_params();
    const std::vector<uint8_t> cls = classify_tokens(p);
    for (unsigned seed = 1; seed <= 3; ++seed) { test_greedy(p, cls, 0, seed); test_greedy(p, cls, 3, seed + 10); }
    test_books();
    test_session_block();
    test_container();
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("all checks passed\n");
    return 0;
}
