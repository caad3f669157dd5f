// Many concurrent streams from one thread, the way a server front end would drive this library: N sessions are fed 100 ms at a
// time through the engine ABI's pipelined group feed (include/aprilx_engine.h aprilx_feed_many_pipelined, depth 2: the call for
// feed k + 1 returns when feed k is complete, so the library prepares and launches a feed while the GPU still works on the one
// before it).  The reference has no counterpart: its sessions are fed one by one (example.cpp) and each runs its own ONNX graphs.
//
//   g++ -O2 -std=c++17 examples/serve_many.cpp -I include -L april_asr_amd -laprilasr -Wl,-rpath,$PWD/april_asr_amd -o serve_many
//   ./serve_many model.april audio.raw [sessions=64] [mode=pipelined|lockstep] [input_rate] [--alternatives K] [--bias FILE [--bias-strict]]
//               [--endpoint-ms N] [--blank-penalty X] [--vad] [--dtmf] [--tones] [--quality] [--migrate S] [--lm FILE [--lm-weight W]]
//
// Every session gets the same PCM16 file, rotated by (session index x 0.37 s) so that the streams differ.  With `input_rate` the file
// is PCM16 at that rate and every session is told so (aprilx_session_set_input_rate): the library converts it to the model's rate on
// the GPU; the feeds stay 100 ms of audio (input_rate / 10 samples).  Prints one line per
// session -- "<index> <callbacks> <final results> <tokens in final results> <text of the last final result>" -- and the wall time.
// `--alternatives K` (anywhere on the line) asks every session for per-token confidences with K alternatives
// (aprilx_session_set_confidence) and adds the mean confidence of the tokens in final results to the timing line.
// `--bias FILE` (anywhere on the line): one "boost<TAB>phrase" per line; every session's search boosts these phrases
// (aprilx_bias_create / aprilx_session_set_bias, one set shared by all sessions); `--bias-sessions N` gives the set to the first N
// sessions only (the others are unbiased neighbours on an engine that has opted in).  `--bias-strict` builds the set as a closed
// phrase list (APRILX_BIAS_STRICT): the sessions that have it emit only sequences of the file's phrases.
// `--lm FILE` (anywhere on the line): FILE is plain text from the caller's domain, one utterance per line, written the way the model's
// tokens are written; the library estimates a byte 5-gram model from it (aprilx_lm_create) and every session's search adds
// W * log P(token text) + B to its non-blank logits (aprilx_session_set_lm; `--lm-weight W`, default 0.3, a placeholder: no accuracy
// has been measured; `--lm-bonus B`, default 0).  `--lm-sessions N` gives the model to the first N sessions only.  A session with a
// model cannot be snapshotted: `--lm` with `--migrate` is refused.
// `--endpoint-ms N` / `--blank-penalty X` (anywhere on the line): every session gets search options (aprilx_session_set_search_options):
// an utterance ends N ms after its last token instead of 2200, X is subtracted from the blank logit in the decision.
// `--vad` (anywhere on the line): every session gets the voice-activity detector with its default options (aprilx_session_set_vad); its line
// then ends with " vad <segments> <speech seconds>", and the timing lines say what a step cost.
// `--dtmf` (anywhere on the line): every session gets the DTMF detector with its default options (aprilx_session_set_dtmf); its line then
// ends with " dtmf <digits>" ("-" when no key was found).
// `--tones` (anywhere on the line): every session gets the tone detector with its default options (aprilx_session_set_tones); its line then
// ends with " tones" and one "<name or f1[+f2]>@<on ms>-<off ms>" per tone ("-" when none was found), the names aprilx_tone_name()'s.
// `--quality` (anywhere on the line): every session gets the line-quality observer with its default options (aprilx_session_set_quality); its
// line then ends with " quality rms <dBFS> peak <dBFS> clipped <frames> dropout <seconds>" over the whole stream ("-inf" for digital
// silence).  A session with the observer cannot be snapshotted: `--quality` with `--migrate` is refused.
// `--migrate S` (anywhere on the line): after S feeds every stream is snapshotted (aprilx_snapshot_many), freed, and restored into a new
// session configured the same way (aprilx_restore_many), then the feeds go on: the printed lines equal those of a run without the flag.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "april_api.h"
#include "aprilx_engine.h"

#include <cmath>

struct Stream {
    size_t calls = 0, finals = 0, final_tokens = 0; std::string last_final; double conf_sum = 0; size_t conf_n = 0;
    size_t vad_segments = 0; uint64_t vad_open_ms = 0, vad_speech_ms = 0;
    std::string dtmf_digits;
    std::string tones; size_t tone_count = 0;
    uint64_t q_sumsq = 0, q_samples = 0, q_clipped = 0, q_drop_open_ms = 0, q_drop_ms = 0; int q_peak = 0;
};

static void on_quality(void *ud, const AprilxQualityEvent *e)
{
    Stream *s = static_cast<Stream *>(ud);
    if (e->kind == APRILX_QUALITY_REPORT) {
        s->q_sumsq += e->sumsq; s->q_samples += (uint64_t)e->frames * e->hop; s->q_clipped += e->clipped_frames;
        s->q_peak = std::max(s->q_peak, std::max(std::abs(e->min), std::abs(e->max)));
    } else if (e->kind == APRILX_QUALITY_DROPOUT_ON) s->q_drop_open_ms = e->time_ms;
    else if (e->kind == APRILX_QUALITY_DROPOUT_OFF) s->q_drop_ms += e->time_ms - s->q_drop_open_ms;
}

static void on_tone(void *ud, int kind, uint32_t f1_hz, uint32_t f2_hz, uint64_t time_ms)
{
    Stream *s = static_cast<Stream *>(ud);
    char buf[64];
    if (kind == APRILX_TONE_ON) {
        const char *name = aprilx_tone_name(f1_hz, f2_hz, 20);
        if (name) snprintf(buf, sizeof buf, " %s@%llu", name, (unsigned long long)time_ms);
        else if (f2_hz) snprintf(buf, sizeof buf, " %u+%u@%llu", f1_hz, f2_hz, (unsigned long long)time_ms);
        else snprintf(buf, sizeof buf, " %u@%llu", f1_hz, (unsigned long long)time_ms);
        s->tone_count++;
    } else snprintf(buf, sizeof buf, "-%llu", (unsigned long long)time_ms);
    s->tones += buf;
}

static void on_dtmf(void *ud, int kind, char digit, uint64_t)
{
    if (kind == APRILX_DTMF_DOWN) static_cast<Stream *>(ud)->dtmf_digits.push_back(digit);
}

static void on_vad(void *ud, int kind, uint64_t time_ms)
{
    Stream *s = static_cast<Stream *>(ud);
    if (kind == APRILX_VAD_SPEECH_START) { s->vad_segments++; s->vad_open_ms = time_ms; }
    else s->vad_speech_ms += time_ms - s->vad_open_ms;
}

static void on_result(void *ud, AprilResultType type, size_t count, const AprilToken *tokens)
{
    Stream *s = static_cast<Stream *>(ud);
    s->calls++;
    if (type != APRIL_RESULT_RECOGNITION_FINAL) return;
    s->finals++; s->final_tokens += count;
    s->last_final.clear();
    for (size_t i = 0; i < count; ++i) {
        s->last_final += tokens[i].token;
        if (const AprilxTokenInfo *info = static_cast<const AprilxTokenInfo *>(tokens[i].reserved)) { s->conf_sum += std::exp((double)info->token_logprob); s->conf_n++; }
    }
}

int main(int argc, char **argv)
{
    int alternatives = 0;
    const char *bias_file = nullptr, *lm_file = nullptr;
    float lm_weight = 0.3f, lm_bonus = 0.0f;
    int lm_sessions = -1;
    int bias_sessions = -1;
    bool bias_strict = false;
    long endpoint_ms = -1;
    const char *blank_penalty = nullptr;
    bool vad = false, dtmf = false, tones = false, quality = false;
    long migrate = -1;
    for (int i = 1; i + 1 < argc; ++i)
        if (!strcmp(argv[i], "--lm") || !strcmp(argv[i], "--lm-weight") || !strcmp(argv[i], "--lm-bonus") || !strcmp(argv[i], "--lm-sessions")) {
            if (!strcmp(argv[i], "--lm")) lm_file = argv[i + 1];
            else if (!strcmp(argv[i], "--lm-weight")) lm_weight = strtof(argv[i + 1], nullptr);
            else if (!strcmp(argv[i], "--lm-bonus")) lm_bonus = strtof(argv[i + 1], nullptr);
            else lm_sessions = atoi(argv[i + 1]);
            for (int j = i; j + 2 < argc; ++j) argv[j] = argv[j + 2];
            argc -= 2;
            i = 0;
        }
    for (int i = 1; i + 1 < argc; ++i)
        if (!strcmp(argv[i], "--migrate")) {
            migrate = atol(argv[i + 1]);
            for (int j = i; j + 2 < argc; ++j) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    for (int i = 1; i < argc; ++i)
        if (!strcmp(argv[i], "--quality")) {
            quality = true;
            for (int j = i; j + 1 < argc; ++j) argv[j] = argv[j + 1];
            argc -= 1;
            break;
        }
    for (int i = 1; i < argc; ++i)
        if (!strcmp(argv[i], "--tones")) {
            tones = true;
            for (int j = i; j + 1 < argc; ++j) argv[j] = argv[j + 1];
            argc -= 1;
            break;
        }
    for (int i = 1; i < argc; ++i)
        if (!strcmp(argv[i], "--dtmf")) {
            dtmf = true;
            for (int j = i; j + 1 < argc; ++j) argv[j] = argv[j + 1];
            argc -= 1;
            break;
        }
    for (int i = 1; i < argc; ++i)
        if (!strcmp(argv[i], "--vad")) {
            vad = true;
            for (int j = i; j + 1 < argc; ++j) argv[j] = argv[j + 1];
            argc -= 1;
            break;
        }
    for (int i = 1; i + 1 < argc; ++i)
        if (!strcmp(argv[i], "--endpoint-ms")) {
            endpoint_ms = atol(argv[i + 1]);
            for (int j = i; j + 2 < argc; ++j) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    for (int i = 1; i + 1 < argc; ++i)
        if (!strcmp(argv[i], "--blank-penalty")) {
            blank_penalty = argv[i + 1];
            for (int j = i; j + 2 < argc; ++j) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    for (int i = 1; i < argc; ++i)
        if (!strcmp(argv[i], "--bias-strict")) {
            bias_strict = true;
            for (int j = i; j + 1 < argc; ++j) argv[j] = argv[j + 1];
            argc -= 1;
            break;
        }
    for (int i = 1; i + 1 < argc; ++i)
        if (!strcmp(argv[i], "--bias-sessions")) {
            bias_sessions = atoi(argv[i + 1]);
            for (int j = i; j + 2 < argc; ++j) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    for (int i = 1; i + 1 < argc; ++i)
        if (!strcmp(argv[i], "--bias")) {
            bias_file = argv[i + 1];
            for (int j = i; j + 2 < argc; ++j) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    for (int i = 1; i + 1 < argc; ++i)
        if (!strcmp(argv[i], "--alternatives")) {
            alternatives = atoi(argv[i + 1]);
            for (int j = i; j + 2 < argc; ++j) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    if (argc < 3) { fprintf(stderr, "usage: %s <model.april> <audio.raw (PCM16 mono)> [sessions=64] [pipelined|lockstep] [input_rate]\n", argv[0]); return 2; }
    const int n = argc > 3 ? atoi(argv[3]) : 64;
    const bool pipelined = !(argc > 4 && !strcmp(argv[4], "lockstep"));
    aam_api_init(APRIL_VERSION);
    AprilASRModel model = aam_create_model(argv[1]);
    if (!model) { fprintf(stderr, "failed to load model %s\n", argv[1]); return 1; }
    FILE *f = fopen(argv[2], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
    std::vector<short> pcm;
    { short buf[4096]; size_t got; while ((got = fread(buf, sizeof(short), 4096, f)) > 0) pcm.insert(pcm.end(), buf, buf + got); }
    fclose(f);
    const size_t rate = argc > 5 ? (size_t)atol(argv[5]) : aam_get_sample_rate(model);      // of the file
    const size_t step = rate / 10;                                       // 100 ms
    const size_t steps = pcm.size() / step;
    if (!steps) { fprintf(stderr, "audio shorter than one feed\n"); return 1; }

    AprilxBias bias = nullptr;
    if (bias_file) {
        FILE *bf = fopen(bias_file, "r");
        if (!bf) { fprintf(stderr, "cannot open %s\n", bias_file); return 1; }
        std::vector<std::string> phrases; std::vector<float> boosts;
        char line[1024];
        for (int ln = 1; fgets(line, sizeof line, bf); ++ln) {
            char *tab = strchr(line, '\t'), *end = nullptr;
            const float boost = strtof(line, &end);
            std::string p(tab ? tab + 1 : "");
            while (!p.empty() && (p.back() == '\n' || p.back() == '\r')) p.pop_back();
            if (!tab || end != tab || end == line || p.empty()) { fprintf(stderr, "%s:%d: expected boost<TAB>phrase\n", bias_file, ln); return 1; }
            boosts.push_back(boost); phrases.push_back(p);
        }
        fclose(bf);
        std::vector<const char *> ptrs;
        for (const std::string &p : phrases) ptrs.push_back(p.c_str());
        char err[256];
        bias = aprilx_bias_create_ex(model, ptrs.size(), ptrs.data(), boosts.data(), bias_strict ? APRILX_BIAS_STRICT : 0u, err, sizeof err);
        if (!bias) { fprintf(stderr, "bias set refused: %s\n", err); return 1; }
        int32_t states = 0; int64_t edges = 0;
        const int dropped = aprilx_bias_info(bias, &states, &edges);
        fprintf(stderr, "bias set%s: %zu phrases (%d left out as unspellable), %d states, %lld token edges\n", bias_strict ? " (strict)" : "", phrases.size(), dropped, states, (long long)edges);
    }
    if (quality && migrate >= 0) { fprintf(stderr, "--quality and --migrate exclude each other: a snapshot does not carry the observer's machine\n"); return 1; }
    AprilxLm lm = nullptr;
    if (lm_file) {
        if (migrate >= 0) { fprintf(stderr, "--lm and --migrate exclude each other: a snapshot does not carry the language model's node\n"); return 1; }
        FILE *lf = fopen(lm_file, "rb");
        if (!lf) { fprintf(stderr, "cannot open %s\n", lm_file); return 1; }
        std::string text;
        char buf[65536];
        for (size_t got; (got = fread(buf, 1, sizeof buf, lf)) > 0;) text.append(buf, got);
        fclose(lf);
        char err[256];
        lm = aprilx_lm_create(model, text.data(), text.size(), 5, err, sizeof err);
        if (!lm) { fprintf(stderr, "language model refused: %s\n", err); return 1; }
        int32_t order = 0, nodes = 0, start = 0, alphabet = 0; int64_t arcs = 0;
        const int dropped = aprilx_lm_info(lm, &order, &nodes, &arcs, &start, &alphabet);
        fprintf(stderr, "language model: order %d, %d nodes, %lld arcs, %d bytes in the alphabet, %d lines left out; weight %.3f, bonus %.3f\n", order, nodes, (long long)arcs, alphabet, dropped,
                lm_weight, lm_bonus);
    }
    std::vector<Stream> streams((size_t)n);
    std::vector<AprilASRSession> sessions((size_t)n);
    std::vector<std::vector<short>> audio((size_t)n);
    // a session for stream i, configured by the command line: at the start, and again for the restored copy of a migrated stream
    auto make_session = [&](int i) -> int {
        AprilConfig cfg;
        memset(&cfg, 0, sizeof cfg);
        cfg.handler = on_result; cfg.userdata = &streams[(size_t)i];
        cfg.flags = APRIL_CONFIG_FLAG_ZERO_BIT;                           // synchronous: handlers run on this thread, inside the feed calls
        sessions[(size_t)i] = aas_create_session(model, cfg);
        if (!sessions[(size_t)i]) { fprintf(stderr, "failed to create session %d\n", i); return 1; }
        if (argc > 5 && aprilx_session_set_input_rate(sessions[(size_t)i], (uint32_t)rate) != 0) { fprintf(stderr, "input rate %zu refused\n", rate); return 1; }
        if (alternatives && aprilx_session_set_confidence(sessions[(size_t)i], alternatives) != 0) { fprintf(stderr, "%d alternatives refused\n", alternatives); return 1; }
        if (bias && (bias_sessions < 0 || i < bias_sessions) && aprilx_session_set_bias(sessions[(size_t)i], bias) != 0) { fprintf(stderr, "bias set refused by session %d\n", i); return 1; }
        if (lm && (lm_sessions < 0 || i < lm_sessions) && aprilx_session_set_lm(sessions[(size_t)i], lm, lm_weight, lm_bonus) != 0) { fprintf(stderr, "language model refused by session %d\n", i); return 1; }
        if (endpoint_ms >= 0 || blank_penalty) {
            AprilxSearchOptions so;
            so.size = (uint32_t)sizeof so; so.endpoint_silence_ms = endpoint_ms >= 0 ? (uint32_t)endpoint_ms : 2200u; so.max_utterance_ms = 0;
            so.blank_penalty = blank_penalty ? strtof(blank_penalty, nullptr) : 0.0f;
            if (aprilx_session_set_search_options(sessions[(size_t)i], &so) != 0) { fprintf(stderr, "search options refused\n"); return 1; }
        }
        if (vad) {
            AprilxVadOptions vo = {(uint32_t)sizeof vo, 200.0f, 4000.0f, 5.0f, 3.0f, 50u, 300u, -12.0f, 0u};
            if (aprilx_session_set_vad(sessions[(size_t)i], &vo, on_vad, &streams[(size_t)i]) != 0) { fprintf(stderr, "voice-activity options refused\n"); return 1; }
        }
        if (dtmf) {
            AprilxDtmfOptions dopt = {(uint32_t)sizeof dopt, -40.0f, 4.0f, 8.0f, 8.0f, 0.6f, 20u, 20u, 0u};
            if (aprilx_session_set_dtmf(sessions[(size_t)i], &dopt, on_dtmf, &streams[(size_t)i]) != 0) { fprintf(stderr, "DTMF options refused\n"); return 1; }
        }
        if (tones) {
            AprilxToneOptions topt = {(uint32_t)sizeof topt, -40.0f, 10.0f, 0.7f, 20u, 60u, 30u, 0u};
            if (aprilx_session_set_tones(sessions[(size_t)i], &topt, on_tone, &streams[(size_t)i]) != 0) { fprintf(stderr, "tone options refused\n"); return 1; }
        }
        if (quality) {
            AprilxQualityOptions qopt = {(uint32_t)sizeof qopt, 0u, 32767u, 3u, 1000u, 200u, 1000u};
            if (aprilx_session_set_quality(sessions[(size_t)i], &qopt, on_quality, &streams[(size_t)i]) != 0) { fprintf(stderr, "quality options refused\n"); return 1; }
        }
        return 0;
    };
    for (int i = 0; i < n; ++i) {
        if (make_session(i) != 0) return 1;
        const size_t rot = ((size_t)i * (size_t)(0.37 * rate)) % pcm.size();
        audio[(size_t)i].assign(pcm.begin() + (long)rot, pcm.end());
        audio[(size_t)i].insert(audio[(size_t)i].end(), pcm.begin(), pcm.begin() + (long)rot);
    }
    std::vector<const short *> ptrs((size_t)n);
    std::vector<size_t> counts((size_t)n, step);
    const auto t0 = std::chrono::steady_clock::now();
    double migrate_ms = 0; size_t migrate_bytes = 0;
    for (size_t k = 0; k < steps; ++k) {
        if (migrate >= 0 && k == (size_t)migrate) {
            // every stream moves: one gather launch per engine, free, create + configure, one scatter launch per engine
            const auto m0 = std::chrono::steady_clock::now();
            if (pipelined) aprilx_drain_many((size_t)n, sessions.data());
            std::vector<int64_t> sizes((size_t)n);
            if (aprilx_snapshot_many((size_t)n, sessions.data(), nullptr, nullptr, sizes.data()) != 0) { fprintf(stderr, "snapshot refused\n"); return 1; }
            std::vector<std::vector<char>> blobs((size_t)n); std::vector<void *> dsts((size_t)n); std::vector<const void *> srcs((size_t)n); std::vector<size_t> caps((size_t)n);
            for (int i = 0; i < n; ++i) { blobs[(size_t)i].resize((size_t)sizes[(size_t)i]); dsts[(size_t)i] = blobs[(size_t)i].data(); srcs[(size_t)i] = dsts[(size_t)i]; caps[(size_t)i] = blobs[(size_t)i].size(); migrate_bytes += caps[(size_t)i]; }
            if (aprilx_snapshot_many((size_t)n, sessions.data(), dsts.data(), caps.data(), sizes.data()) != 0) { fprintf(stderr, "snapshot refused\n"); return 1; }
            for (AprilASRSession s : sessions) aas_free(s);
            for (int i = 0; i < n; ++i) if (make_session(i) != 0) return 1;
            std::vector<int> status((size_t)n);
            if (aprilx_restore_many((size_t)n, sessions.data(), srcs.data(), caps.data(), status.data()) != 0) { fprintf(stderr, "restore refused\n"); return 1; }
            migrate_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - m0).count();
        }
        for (int i = 0; i < n; ++i) ptrs[(size_t)i] = audio[(size_t)i].data() + k * step;
        if (pipelined) aprilx_feed_many_pipelined((size_t)n, sessions.data(), ptrs.data(), counts.data(), 2);
        else aprilx_feed_many((size_t)n, sessions.data(), ptrs.data(), counts.data());
    }
    if (pipelined) aprilx_drain_many((size_t)n, sessions.data());
    aprilx_flush_many((size_t)n, sessions.data());
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (int i = 0; i < n; ++i) {
        const Stream &s = streams[(size_t)i];
        printf("%d %zu %zu %zu %s", i, s.calls, s.finals, s.final_tokens, s.last_final.c_str());
        if (vad) printf(" vad %zu %.2f", s.vad_segments, (double)s.vad_speech_ms * 1e-3);      // (the flush has closed every open segment)
        if (dtmf) printf(" dtmf %s", s.dtmf_digits.empty() ? "-" : s.dtmf_digits.c_str());
        if (tones) printf(" tones%s", s.tones.empty() ? " -" : s.tones.c_str());      // (the flush has closed every held tone)
        if (quality) {                                 // (the flush has closed the last interval and an open dropout)
            const double rms = s.q_samples && s.q_sumsq ? 10.0 * std::log10((double)s.q_sumsq / (double)s.q_samples / (32768.0 * 32768.0)) : -INFINITY;
            const double peak = s.q_peak ? 20.0 * std::log10((double)s.q_peak / 32768.0) : -INFINITY;
            printf(" quality rms %.1f peak %.1f clipped %llu dropout %.2f", rms, peak, (unsigned long long)s.q_clipped, (double)s.q_drop_ms * 1e-3);
        }
        printf("\n");
    }
    fprintf(stderr, "%d streams x %.1f s of audio in %.1f ms (%s feed): %.0f audio-seconds per second\n", n, steps * 0.1, ms, pipelined ? "pipelined" : "lock-step",
            n * steps * 0.1 / (ms * 1e-3));
    if (migrate >= 0) fprintf(stderr, "migrated %d streams after %ld feeds: %.1f KB per stream, %.2f ms for snapshot, free, create and restore of all\n", n, migrate,
                              migrate_bytes / 1024.0 / n, migrate_ms);
    if (alternatives) {
        double sum = 0; size_t cnt = 0;
        for (const Stream &s : streams) { sum += s.conf_sum; cnt += s.conf_n; }
        fprintf(stderr, "%d alternatives: %.3f ms per 100 ms step, mean confidence of %zu final tokens %.3f\n", alternatives, ms / (double)steps, cnt, cnt ? sum / (double)cnt : 0.0);
    }
    if (bias) fprintf(stderr, "phrase boosting: %.3f ms per 100 ms step\n", ms / (double)steps);
    if (lm) {
        uint64_t launches = 0, uploads = 0; int32_t resident = 0;
        aprilx_model_lm_stats(model, 0, &launches, &resident, &uploads);
        fprintf(stderr, "language model: %.3f ms per 100 ms step, %llu decision launches of the LM forms issued, %d model(s) resident on device 0\n", ms / (double)steps,
                (unsigned long long)launches, resident);
    }
    if (endpoint_ms >= 0 || blank_penalty) fprintf(stderr, "search options: %.3f ms per 100 ms step\n", ms / (double)steps);
    if (vad) {
        uint64_t launches = 0, frames = 0; double kms = 0; size_t segs = 0; double secs = 0;
        aprilx_model_vad_stats(model, 0, &launches, &frames, &kms);
        for (const Stream &s : streams) { segs += s.vad_segments; secs += (double)s.vad_speech_ms * 1e-3; }
        fprintf(stderr, "voice activity: %.3f ms per 100 ms step, %zu segments, %.1f speech seconds, %llu launches over %llu frames on device 0\n", ms / (double)steps, segs, secs,
                (unsigned long long)launches, (unsigned long long)frames);
    }
    if (dtmf) {
        uint64_t launches = 0, frames = 0; double kms = 0; size_t keys = 0;
        aprilx_model_dtmf_stats(model, 0, &launches, &frames, &kms);
        for (const Stream &s : streams) keys += s.dtmf_digits.size();
        fprintf(stderr, "DTMF: %.3f ms per 100 ms step, %zu keys, %llu launches over %llu frames on device 0\n", ms / (double)steps, keys,
                (unsigned long long)launches, (unsigned long long)frames);
    }
    if (quality) {
        uint64_t launches = 0, frames = 0; double kms = 0;
        aprilx_model_quality_stats(model, 0, &launches, &frames, &kms);
        fprintf(stderr, "quality: %.3f ms per 100 ms step, %llu launches over %llu frames on device 0\n", ms / (double)steps, (unsigned long long)launches,
                (unsigned long long)frames);
    }
    if (tones) {
        uint64_t launches = 0, frames = 0; double kms = 0; size_t found = 0;
        aprilx_model_tone_stats(model, 0, &launches, &frames, &kms);
        for (const Stream &s : streams) found += s.tone_count;
        fprintf(stderr, "tones: %.3f ms per 100 ms step, %zu tones, %llu launches over %llu frames on device 0\n", ms / (double)steps, found,
                (unsigned long long)launches, (unsigned long long)frames);
    }
    if (argc > 5) fprintf(stderr, "input at %zu Hz: %.3f ms per 100 ms step\n", rate, ms / (double)steps);
    for (AprilASRSession s : sessions) aas_free(s);
    if (bias) aprilx_bias_free(bias);
    if (lm) aprilx_lm_free(lm);
    aam_free(model);
    return 0;
}
