// A C client of the per-token confidences (include/aprilx_engine.h aprilx_session_set_confidence), in the style of
// examples/main.cpp: one synchronous session with K = 3 fed 100 ms at a time, then flushed.  Its handler reads
// AprilToken.reserved and prints, per result, "<type> <count>" and per token
// "<id> <bits of token_logprob> <bits of blank_logprob> <eval_index> <n_alt>".  tests/test_gpu_confidence.py compares the
// output with what the Python binding delivers for the same file.
//
//   confidence_client model.april audio.raw
#include <cstdio>
#include <cstring>
#include <vector>
#include "april_api.h"
#include "aprilx_engine.h"

static int bad = 0;

static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }

static void on_result(void *, AprilResultType type, size_t count, const AprilToken *tokens)
{
    printf("%d %zu\n", (int)type, count);
    for (size_t i = 0; i < count; ++i) {
        const AprilxTokenInfo *info = static_cast<const AprilxTokenInfo *>(tokens[i].reserved);
        if (!info || info->size != sizeof(AprilxTokenInfo)) { bad++; continue; }
        printf("%d %08x %08x %llu %u\n", info->alt_id[0], bits(info->token_logprob), bits(info->blank_logprob), (unsigned long long)info->eval_index, info->n_alt);
    }
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s <model.april> <audio.raw (PCM16 mono)>\n", argv[0]); return 2; }
    aam_api_init(APRIL_VERSION);
    AprilASRModel model = aam_create_model(argv[1]);
    if (!model) { fprintf(stderr, "failed to load model %s\n", argv[1]); return 1; }
    FILE *f = fopen(argv[2], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
    std::vector<short> pcm;
    { short buf[4096]; size_t got; while ((got = fread(buf, sizeof(short), 4096, f)) > 0) pcm.insert(pcm.end(), buf, buf + got); }
    fclose(f);
    AprilConfig cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.handler = on_result;
    cfg.flags = APRIL_CONFIG_FLAG_ZERO_BIT;
    AprilASRSession session = aas_create_session(model, cfg);
    if (!session) { fprintf(stderr, "failed to create a session\n"); return 1; }
    if (aprilx_session_set_confidence(session, 9) != -1 || aprilx_session_set_confidence(session, 3) != 0 || aprilx_session_confidence(session) != 3) {
        fprintf(stderr, "aprilx_session_set_confidence misbehaves\n");
        return 1;
    }
    const size_t step = aam_get_sample_rate(model) / 10;
    for (size_t o = 0; o < pcm.size(); o += step) aas_feed_pcm16(session, pcm.data() + o, pcm.size() - o < step ? pcm.size() - o : step);
    if (aprilx_session_set_confidence(session, 0) != -1) { fprintf(stderr, "the option was accepted in the middle of a segment\n"); return 1; }
    aas_flush(session);
    aas_free(session);
    aam_free(model);
    if (bad) { fprintf(stderr, "%d tokens without an AprilxTokenInfo\n", bad); return 1; }
    return 0;
}
