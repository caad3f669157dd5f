// Stand-alone check of csrc/input_format.h under AddressSanitizer + UBSan (tests/test_input_format_cpu.py builds and runs it):
//   * the host decode over every format at odd source offsets and zero lengths, from heap blocks of exactly the bytes it may read,
//     against the same frames decoded from an aligned copy and against the contract's literal values;
//   * the raw-byte queue of a formatted session (RawFifo: append, absorb, settle, drop, span) against a plain re-statement -- one
//     byte vector and an index -- under random operation sequences, with lent buffers that are freed as soon as the queue must
//     no longer read them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>
#include "input_format.h"

using namespace aprilx;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static InputFormat fmt(uint32_t enc, uint32_t ch, int32_t c)
{
    InputFormat f; f.encoding = enc; f.channels = ch; f.channel = c; f.frame_bytes = ch * encoding_bytes(enc);
    return f;
}

static void literals()
{
    CHECK(decode_mulaw(0xFF) == 0 && decode_mulaw(0x7F) == 0 && decode_mulaw(0x00) == -32124 && decode_mulaw(0x80) == 32124);
    CHECK(decode_alaw(0xD5) == 8 && decode_alaw(0x55) == -8 && decode_alaw(0x2A) == -32256 && decode_alaw(0xAA) == 32256);
    CHECK(decode_f32(0.5f / 32768.0f) == 0 && decode_f32(1.5f / 32768.0f) == 2 && decode_f32(2.5f / 32768.0f) == 2 && decode_f32(-1.5f / 32768.0f) == -2);
    CHECK(decode_f32(1.0f) == 32767 && decode_f32(-1.0f) == -32768 && decode_f32(-0.0f) == 0 && decode_f32(1e-40f) == 0);
    CHECK(decode_f32(__builtin_inff()) == 32767 && decode_f32(-__builtin_inff()) == -32768 && decode_f32(__builtin_nanf("")) == 0);
    CHECK(decode_f32(3.0e38f) == 32767 && decode_f32(-3.0e38f) == -32768);
    CHECK(downmix(1, 2) == 1 && downmix(-1, 2) == 0 && downmix(-3, 2) == -1);
    CHECK(downmix(8 * 32767, 8) == 32767 && downmix(-8 * 32768, 8) == -32768);
    for (int b = 0; b < 256; ++b) {
        CHECK(decode_mulaw((uint32_t)b) == -decode_mulaw((uint32_t)b ^ 0x80u));
        CHECK(decode_alaw((uint32_t)b) == -decode_alaw((uint32_t)b ^ 0x80u));
    }
}

// every format, frame counts 0 .. 9 and 257, source offsets 0 .. 7: the frames sit at the END of a heap block of exactly
// offset + bytes bytes, so a read past them (or a wider read at an odd address) is a sanitizer report
static void offsets(std::mt19937 &rng)
{
    const int counts[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 257};
    for (uint32_t enc = 0; enc < ENC_COUNT; ++enc)
        for (uint32_t ch : {1u, 2u, 3u, 8u})
            for (int32_t c : {-1, 0, (int32_t)ch - 1})
                for (int n : counts)
                    for (size_t off = 0; off < 8; ++off) {
                        const InputFormat f = fmt(enc, ch, c);
                        const size_t bytes = (size_t)n * f.frame_bytes;
                        std::vector<uint8_t> aligned(bytes);
                        for (uint8_t &b : aligned) b = (uint8_t)rng();
                        std::unique_ptr<uint8_t[]> block(new uint8_t[off + bytes]);
                        if (bytes) memcpy(block.get() + off, aligned.data(), bytes);
                        for (int i = 0; i < n; ++i) {
                            const int16_t got = decode_frame(f, block.get() + off + (size_t)i * f.frame_bytes);
                            // the re-statement: the frame's values from the aligned copy, typed loads, 64-bit arithmetic
                            int64_t s = 0, pick = 0;
                            for (uint32_t k = 0; k < ch; ++k) {
                                int64_t v;
                                const uint8_t *p = aligned.data() + (size_t)i * f.frame_bytes;
                                if (enc == ENC_S16) { int16_t t; memcpy(&t, p + 2 * k, 2); v = t; }
                                else if (enc == ENC_F32) { float t; memcpy(&t, p + 4 * k, 4); v = decode_f32(t); }
                                else v = enc == ENC_MULAW ? decode_mulaw(p[k]) : decode_alaw(p[k]);
                                s += v;
                                if ((int32_t)k == c) pick = v;
                            }
                            int64_t want = pick;
                            if (c < 0) { const int64_t num = 2 * s + ch, den = 2 * (int64_t)ch; want = num / den - ((num % den != 0 && num < 0) ? 1 : 0); }
                            CHECK(want >= -32768 && want <= 32767);
                            CHECK(got == (int16_t)want);
                        }
                    }
}

// the plain re-statement of the queue: every byte ever appended and not yet dropped, in order
struct Plain { std::vector<uint8_t> all; };

static void fifo_ops(std::mt19937 &rng, size_t fbytes)
{
    RawFifo q; q.fbytes = fbytes;
    Plain ref;
    std::unique_ptr<uint8_t[]> lent;          // the caller's buffer while it is lent
    auto frames = [&](size_t n) { std::vector<uint8_t> v(n * fbytes); for (uint8_t &b : v) b = (uint8_t)rng(); return v; };
    auto same = [&] {
        CHECK(q.count() * fbytes == ref.all.size());
        if (!q.count()) return;
        // the whole queue, and a random inner span, as parts
        for (int k = 0; k < 2; ++k) {
            size_t l0 = 0, l1 = q.count();
            if (k) { l0 = rng() % q.count(); l1 = l0 + 1 + rng() % (q.count() - l0); }
            RawFifo::Parts parts;
            q.span(l0, l1, parts);
            CHECK(parts.size() >= 1 && parts.size() <= 2);
            std::vector<uint8_t> got;
            for (auto &p : parts) got.insert(got.end(), p.first, p.first + p.second);
            CHECK(got.size() == (l1 - l0) * fbytes && memcmp(got.data(), ref.all.data() + l0 * fbytes, got.size()) == 0);
        }
    };
    for (int step = 0; step < 400; ++step) {
        const int op = (int)(rng() % 6);
        if (op == 0) {                                          // a copied feed (0 .. 40 frames): behind a lent buffer only after absorb
            const std::vector<uint8_t> v = frames(rng() % 41);
            q.absorb(); lent.reset();
            q.append(v.data(), v.size() / fbytes);
            ref.all.insert(ref.all.end(), v.begin(), v.end());
        } else if (op == 1 && !q.ext) {                         // a lent feed (1 .. 40 frames) in a heap block of exactly its size
            const std::vector<uint8_t> v = frames(1 + rng() % 40);
            lent.reset(new uint8_t[v.size()]);
            memcpy(lent.get(), v.data(), v.size());
            q.ext = lent.get(); q.ext_cnt = v.size() / fbytes;
            ref.all.insert(ref.all.end(), v.begin(), v.end());
        } else if (op == 2) {                                   // absorb: the lent buffer may go at once
            q.absorb(); lent.reset();
        } else if (op == 3) {                                   // settle at a random keep point: afterwards the lent buffer is never read again
            const size_t keep = q.count() ? rng() % (q.count() + 1) : 0;
            const bool had = q.ext != nullptr;
            const size_t own = q.own();
            const bool moved = q.settle(keep);
            CHECK(moved == (had && keep >= own));
            CHECK(q.ext == nullptr && q.ext_cnt == 0);
            lent.reset();
            if (moved) ref.all.erase(ref.all.begin(), ref.all.begin() + (long)(keep * fbytes));
        } else if (op == 4 && !q.ext) {                         // compact: drop consumed frames from the front
            const size_t n = q.own() ? rng() % (q.own() + 1) : 0;
            q.drop(n);
            ref.all.erase(ref.all.begin(), ref.all.begin() + (long)(n * fbytes));
        } else if (op == 5 && rng() % 8 == 0) {
            q.clear(); lent.reset(); ref.all.clear();
        }
        same();
    }
}

int main()
{
    std::mt19937 rng(20240611);
    literals();
    offsets(rng);
    for (size_t fb : {1u, 2u, 3u, 4u, 6u, 12u, 32u}) fifo_ops(rng, fb);
    if (fails) { printf("%d checks failed\n", fails); return 1; }
    printf("all checks passed\n");
    return 0;
}
