// See engine.h.
#include "engine.h"
#include <array>
#include <algorithm>
#include <cmath>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <thread>
#include "common.h"
#include "env.h"
#include "rowepi_forms.h"

namespace aprilx {

// ---------------------------------------------------------------- packing
static size_t align64(size_t x) { return (x + 63) & ~(size_t)63; }

void plan_layout(const NetDims &d, bool has_dec_conv_b, PackedLayout &L)
{
    L.dims = d;
    L.has_dec_conv_b = has_dec_conv_b;
    L.vocab_pad = (d.vocab + 31) & ~31;            // a multiple of 32: the joiner GEMM's full-K tiles are 32 columns wide
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off = align64(off + n); return o; };
    // conv 0/1: OIHW as exported; conv 2 runs as an im2col GEMM: MFMA-packed [k3][conv_ch[2]], k = ci*9 + i*3 + j
    L.k3 = (d.conv_ch[1] * 9 + 63) & ~63;          // K of every GEMM is a multiple of 64 (4 waves x 16-wide blocks)
    L.conv_w[0] = take((size_t)d.conv_ch[0] * 9); L.conv_b[0] = take((size_t)d.conv_ch[0]);
    L.conv_w[1] = take((size_t)d.conv_ch[1] * d.conv_ch[0] * 9); L.conv_b[1] = take((size_t)d.conv_ch[1]);
    L.conv_w[2] = take((size_t)L.k3 * d.conv_ch[2]); L.conv_b[2] = take((size_t)d.conv_ch[2]);
    L.w_embed = take((size_t)d.embed_in * d.d_model); L.b_embed = take((size_t)d.d_model);
    L.layers.resize((size_t)d.n_layers);
    for (auto &l : L.layers) {
        l.wg = take((size_t)2 * d.d_model * 4 * d.hidden); l.bg = take((size_t)4 * d.hidden);
        l.whr = take((size_t)d.hidden * d.d_model);
        l.wff1 = take((size_t)d.d_model * d.ffn); l.bff1 = take((size_t)d.ffn);
        l.wff2 = take((size_t)d.ffn * d.d_model); l.bff2 = take((size_t)d.d_model);
    }
    L.w_encproj = take((size_t)d.d_model * d.joiner); L.b_encproj = take((size_t)d.joiner);
    L.emb = take((size_t)d.vocab * d.d_model);
    L.dec_conv = take((size_t)d.d_model * (d.d_model / d.dec_groups) * d.context);
    L.dec_conv_b = take((size_t)d.d_model);
    L.w_decproj = take((size_t)d.d_model * d.joiner); L.b_decproj = take((size_t)d.joiner);
    L.w_out = take((size_t)d.joiner * L.vocab_pad); L.b_out = take((size_t)L.vocab_pad);
    L.total = off;
}

std::vector<std::pair<size_t, size_t>> gemm_sections(const PackedLayout &L)
{
    const NetDims &d = L.dims;
    std::vector<std::pair<size_t, size_t>> v;
    v.emplace_back(L.w_embed, (size_t)d.embed_in * d.d_model);
    for (const PackedLayout::Layer &o : L.layers) {
        v.emplace_back(o.wg, (size_t)2 * d.d_model * 4 * d.hidden); v.emplace_back(o.whr, (size_t)d.hidden * d.d_model);
        v.emplace_back(o.wff1, (size_t)d.d_model * d.ffn); v.emplace_back(o.wff2, (size_t)d.ffn * d.d_model);
    }
    v.emplace_back(L.w_encproj, (size_t)d.d_model * d.joiner); v.emplace_back(L.w_decproj, (size_t)d.d_model * d.joiner);
    v.emplace_back(L.w_out, (size_t)d.joiner * L.vocab_pad);
    return v;
}

// W is K x N row-major; see kernels.h for the packed order.  colmap (optional) gives, for each
// packed column, the source column.
static void pack_mfma(const float *W, int K, int N, int Npad, const std::vector<int> *colmap, float *dst)
{
    const int KB = K / 16, NTt = Npad / 16;
    for (int t = 0; t < NTt; ++t)
        for (int kb = 0; kb < KB; ++kb)
            for (int lane = 0; lane < 64; ++lane) {
                const int np = t * 16 + (lane & 15);
                const int src = np < N ? (colmap ? (*colmap)[(size_t)np] : np) : -1;
                float *o = dst + (((size_t)t * KB + kb) * 64 + lane) * 4;
                for (int j = 0; j < 4; ++j) {
                    const int k = kb * 16 + (lane >> 4) * 4 + j;
                    o[j] = src >= 0 ? W[(size_t)k * N + src] : 0.0f;
                }
            }
}

void pack_weights(const HostModel &m, PackedLayout &L, std::vector<float> &blob)
{
    const NetDims &d = L.dims;
    blob.assign(L.total, 0.0f);
    float *B = blob.data();
    for (int i = 0; i < 3; ++i) {
        if (i < 2) memcpy(B + L.conv_w[i], m.conv_w[i].data(), m.conv_w[i].size() * 4);
        memcpy(B + L.conv_b[i], m.conv_b[i].data(), m.conv_b[i].size() * 4);
    }
    {   // third conv as a K x N matrix: W3[k][o] = w[o][ci][i][j], k = ci*9 + i*3 + j (zero rows up to k3)
        const int kreal = d.conv_ch[1] * 9, c2 = d.conv_ch[2];
        std::vector<float> w3((size_t)L.k3 * c2, 0.0f);
        for (int o = 0; o < c2; ++o) for (int k = 0; k < kreal; ++k) w3[(size_t)k * c2 + o] = m.conv_w[2][(size_t)o * kreal + k];
        pack_mfma(w3.data(), L.k3, c2, c2, nullptr, B + L.conv_w[2]);
    }
    {   // the conv GEMM leaves its output position-major ([f][c]); the graph flattens channel-major (c*f_out + f):
        // permute the embed linear's input rows instead of transposing activations
        const int c2 = d.conv_ch[2], F = d.f_out;
        std::vector<float> we((size_t)d.embed_in * d.d_model);
        for (int c = 0; c < c2; ++c) for (int f = 0; f < F; ++f)
            memcpy(&we[((size_t)f * c2 + c) * d.d_model], &m.w_embed[((size_t)c * F + f) * d.d_model], (size_t)d.d_model * 4);
        pack_mfma(we.data(), d.embed_in, d.d_model, d.d_model, nullptr, B + L.w_embed);
    }
    memcpy(B + L.b_embed, m.b_embed.data(), (size_t)d.d_model * 4);
    L.embed_eps = m.embed_norm_eps;
    L.norm_eps.resize((size_t)d.n_layers);
    // gate columns become unit-major: packed column u*4+g <- source column g*hidden+u
    std::vector<int> gmap((size_t)4 * d.hidden);
    for (int u = 0; u < d.hidden; ++u) for (int g = 0; g < 4; ++g) gmap[(size_t)u * 4 + g] = g * d.hidden + u;
    for (int l = 0; l < d.n_layers; ++l) {
        const LayerWeights &lw = m.layers[(size_t)l];
        const PackedLayout::Layer &o = L.layers[(size_t)l];
        pack_mfma(lw.w_gates.data(), 2 * d.d_model, 4 * d.hidden, 4 * d.hidden, &gmap, B + o.wg);
        for (int n = 0; n < 4 * d.hidden; ++n) B[o.bg + n] = lw.b_gates[(size_t)gmap[(size_t)n]];
        pack_mfma(lw.w_hr.data(), d.hidden, d.d_model, d.d_model, nullptr, B + o.whr);
        pack_mfma(lw.w_ff1.data(), d.d_model, d.ffn, d.ffn, nullptr, B + o.wff1);
        memcpy(B + o.bff1, lw.b_ff1.data(), (size_t)d.ffn * 4);
        pack_mfma(lw.w_ff2.data(), d.ffn, d.d_model, d.d_model, nullptr, B + o.wff2);
        memcpy(B + o.bff2, lw.b_ff2.data(), (size_t)d.d_model * 4);
        L.norm_eps[(size_t)l] = lw.norm_eps;
    }
    pack_mfma(m.w_encproj.data(), d.d_model, d.joiner, d.joiner, nullptr, B + L.w_encproj);
    memcpy(B + L.b_encproj, m.b_encproj.data(), (size_t)d.joiner * 4);
    memcpy(B + L.emb, m.emb.data(), m.emb.size() * 4);
    memcpy(B + L.dec_conv, m.dec_conv.data(), m.dec_conv.size() * 4);
    if (!m.dec_conv_b.empty()) memcpy(B + L.dec_conv_b, m.dec_conv_b.data(), m.dec_conv_b.size() * 4);
    pack_mfma(m.w_decproj.data(), d.d_model, d.joiner, d.joiner, nullptr, B + L.w_decproj);
    memcpy(B + L.b_decproj, m.b_decproj.data(), (size_t)d.joiner * 4);
    pack_mfma(m.w_out.data(), d.joiner, d.vocab, L.vocab_pad, nullptr, B + L.w_out);
    memcpy(B + L.b_out, m.b_out.data(), (size_t)d.vocab * 4);
}

// ---------------------------------------------------------------- engine
// (every allocation holds the process-wide legacy lock, engine.h: an allocation of one engine's stepping thread -- staging regrowth, a
// new launch plan -- must not coincide with another engine's graph capture; recursive, so the constructor's own guard nests)
template <typename T> static T *dmalloc(size_t n) { HipLegacyLock legacy; T *p = nullptr; HIP_CHECK(hipMalloc((void **)&p, std::max<size_t>(n, 1) * sizeof(T))); return p; }
template <typename T> static T *hmalloc(size_t n) { HipLegacyLock legacy; T *p = nullptr; HIP_CHECK(hipHostMalloc((void **)&p, std::max<size_t>(n, 1) * sizeof(T), hipHostMallocDefault)); return p; }

template <typename T> void DeviceTable<T>::alloc(size_t count, const T &off)
{
    n = count; d = dmalloc<T>(n); h = hmalloc<T>(n);
    for (size_t i = 0; i < n; ++i) h[i] = off;
}
template <typename T> void DeviceTable<T>::upload(hipStream_t st) const { HIP_CHECK(hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, st)); }
template <typename T> void DeviceTable<T>::release()
{
    if (d) (void)hipFree(d);
    if (h) (void)hipHostFree(h);
    d = h = nullptr; n = 0;
}

// The device scratch of one debug call: freed when the call leaves, whichever way
struct DeviceScratch {
    std::vector<void *> ptrs;
    DeviceScratch() = default;
    DeviceScratch(const DeviceScratch &) = delete;
    DeviceScratch &operator=(const DeviceScratch &) = delete;
    ~DeviceScratch() { for (void *p : ptrs) (void)hipFree(p); }
    void adopt(void *p) { ptrs.push_back(p); }
    template <typename T> T *alloc(size_t n) { T *p = dmalloc<T>(n); ptrs.push_back(p); return p; }
    template <typename T> T *zeros(size_t n) { T *p = alloc<T>(n); HIP_CHECK(hipMemset(p, 0, std::max<size_t>(n, 1) * sizeof(T))); return p; }
    template <typename T> T *upload(const T *src, size_t n) { T *p = alloc<T>(n); if (n) HIP_CHECK(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice)); return p; }
};

// A debug launch on a stream of its own: live sessions' work on the engine's streams is neither waited for nor delayed
template <typename Launch> static void run_on_private_stream(Launch &&launch)
{
    hipStream_t st = nullptr;
    HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    launch(st);
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipStreamDestroy(st));
}

std::recursive_mutex &hip_legacy_mutex() { static std::recursive_mutex m; return m; }

static int pick_kz(int K, int N, int kblk = 16)
{
    int kz = 256 / std::max(1, N / 16);
    kz = std::max(1, std::min(kz, 8));
    while (kz > 1 && ((K / kblk) / kz < 4 || (K / kblk) % (4 * kz) != 0)) kz >>= 1;   // every wave gets whole blocks of every slab
    return kz;
}

Engine::Engine(const EngineConfig &cfg, const PackedLayout &layout, const float *blob_host, const float *blob_device,
               const ModelParams &params, const FbankHostTables &ft, const std::vector<uint8_t> &tok_class)
    : cfg_(cfg), L_(layout), P_(params)
{
    HipLegacyLock legacy;                      // (allocations, memsets and copies on the legacy stream: not while another engine captures a graph)
    HIP_CHECK(hipSetDevice(cfg_.device));
    HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    HIP_CHECK(hipStreamCreateWithFlags(&f_stream_, hipStreamNonBlocking));
    HIP_CHECK(hipStreamCreateWithFlags(&s_stream_, hipStreamNonBlocking));
    search_stream_ = stream_;
    for (int i = 0; i < 32; ++i) { hipEvent_t e; HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); join_ev_.push_back(e); }
    split_streams_ = std::max(0, std::min(2, env_int("APRIL_SPLIT_STREAMS", 2)));
    const NetDims &d = L_.dims;
    w_ = dmalloc<float>(L_.total);
    if (blob_device) HIP_CHECK(hipMemcpy(w_, blob_device, L_.total * 4, hipMemcpyDeviceToDevice));
    else if (blob_host) HIP_CHECK(hipMemcpy(w_, blob_host, L_.total * 4, hipMemcpyHostToDevice));
    // (neither: the caller fills weights_mut() -- peer copy or RCCL broadcast -- and then calls finish_weights())

    const size_t S = (size_t)cfg_.max_slots, MB = (size_t)cfg_.max_batch;
    // Feature ring per session.  The reference keeps segment_size * 32 frames (src/fbank.c:147); a session that is fed faster
    // than real time (a whole file in one call) is processed a ring's worth of chunks at a time, and the offline wavefront
    // (run_lm_wavefront) needs many more blocks of time steps than layers to fill: 8192 frames = ~80 s of audio per pass
    // (a minute of audio in one call is ONE wavefront: 65.7 ms against 68.8 ms in three passes of a 2048-frame ring),
    // 2.6 MB per slot (10.7 GB at 4096 slots, 3.7 % of this GPU's memory).  Results do not depend on the ring size.
    ring_frames_ = std::max(P_.segment_size * 32, env_int("APRIL_RING_FRAMES", 8192));
    h_ = dmalloc<float>((size_t)d.n_layers * S * d.d_model);
    c_ = dmalloc<float>((size_t)d.n_layers * S * d.hidden);
    if (!env_str("APRIL_RING_FRAMES")) {
        // the default ring is sized for this GPU's 288 GB (10.7 GB at 4096 slots); where that is more than a quarter of what the
        // device has free right now -- several models / lanes / ranks on one device, a smaller GPU -- the ring shrinks (more
        // passes per long feed, same results), so that the allocations that FOLLOW it (state, work buffers, fp16 copies,
        // decoder table) still fit: those abort the process when they fail
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0) {
            const size_t per_frame = S * (size_t)d.mel * sizeof(float);
            const size_t fit = (free_b / 4) / per_frame;
            if (fit < (size_t)ring_frames_) {
                const int shrunk = std::max(P_.segment_size * 32, (int)std::min<size_t>(fit, 8192) / 64 * 64);
                LOGW("engine: %zu MB of feature rings (%d frames x %zu slots) exceed a quarter of the %zu MB free on device %d: %d frames per session",
                     per_frame * (size_t)ring_frames_ >> 20, ring_frames_, S, free_b >> 20, cfg_.device, shrunk);
                ring_frames_ = shrunk;
            }
        } else (void)hipGetLastError();
        float *p = nullptr;
        if (hipMalloc((void **)&p, S * ring_frames_ * d.mel * sizeof(float)) == hipSuccess) ring_ = p;
        else {
            (void)hipGetLastError();
            const size_t asked = S * (size_t)ring_frames_ * d.mel * sizeof(float);
            ring_frames_ = std::max(P_.segment_size * 32, 2048);
            LOGW("engine: no room for %zu MB of feature rings, falling back to %d frames per session", asked >> 20, ring_frames_);
        }
    }
    if (!ring_) ring_ = dmalloc<float>(S * ring_frames_ * d.mel);
    eout_ = dmalloc<float>(S * d.joiner);
    dout_ = dmalloc<float>(S * d.joiner);
    gstate_ = dmalloc<GreedyState>(S);
    HIP_CHECK(hipMemset(h_, 0, (size_t)d.n_layers * S * d.d_model * 4));
    HIP_CHECK(hipMemset(c_, 0, (size_t)d.n_layers * S * d.hidden * 4));
    HIP_CHECK(hipMemset(ring_, 0, S * ring_frames_ * d.mel * 4));
    HIP_CHECK(hipMemset(eout_, 0, S * d.joiner * 4));
    HIP_CHECK(hipMemset(dout_, 0, S * d.joiner * 4));
    {   // every slot starts with context [blank, blank] (april_session.c:432-438), no emission yet (:64-66)
        std::vector<GreedyState> init(S);
        for (auto &g : init) { g.ctx0 = P_.blank_id; g.ctx1 = P_.blank_id; g.last_tok = -1; g.last_emit_ms = 0; }
        HIP_CHECK(hipMemcpy(gstate_, init.data(), S * sizeof(GreedyState), hipMemcpyHostToDevice));
    }
    cls_ = dmalloc<uint8_t>((size_t)d.vocab);
    HIP_CHECK(hipMemcpy(cls_, tok_class.data(), (size_t)d.vocab, hipMemcpyHostToDevice));

    kz_embed_ = pick_kz(d.embed_in, d.d_model);
    kz_hr_ = pick_kz(d.hidden, d.d_model);
    kz_ff2_ = pick_kz(d.ffn, d.d_model);
    kz_proj_ = pick_kz(d.d_model, d.joiner);
    kz_out_ = pick_kz(d.joiner, L_.vocab_pad);
    {   // fp16 tile path: all four layer GEMMs must cut into 4 chunks of whole 32-k blocks (and the gates' y half into whole stages)
        const bool want = cfg_.precision == 1 && env_int("APRIL_F16_TILE", 1) != 0;
        f16_tile_ = want && d.d_model % 128 == 0 && d.hidden % 128 == 0 && d.ffn % 128 == 0 && d.hidden % 16 == 0;
        if (f16_tile_) {
            kzx_hr_ = pick_kz(d.hidden, d.d_model, 32); kzx_ff2_ = pick_kz(d.ffn, d.d_model, 32);
            for (int p = 0; p < 2; ++p) y16_buf_[p] = dmalloc<uint16_t>(MB * d.d_model);
            y16_ = y16_buf_[0];
            for (int p = 0; p < 2; ++p) { xb16_buf_[p] = dmalloc<uint16_t>(MB * d.d_model); u16_buf_[p] = dmalloc<uint16_t>(MB * d.hidden); ff16_buf_[p] = dmalloc<uint16_t>(MB * d.ffn); }
            xb16_ = xb16_buf_[0]; u16_ = u16_buf_[0]; ff16_ = ff16_buf_[0];
            h16_ = dmalloc<uint16_t>((size_t)d.n_layers * S * d.d_model);
            HIP_CHECK(hipMemset(h16_, 0, (size_t)d.n_layers * S * d.d_model * 2));
        }
    }
    ws_mstride_ = cfg_.max_batch;
    const size_t ws_n = (size_t)std::max({kz_embed_ * d.d_model, kz_hr_ * d.d_model, kz_ff2_ * d.d_model, kz_proj_ * d.joiner, kz_out_ * L_.vocab_pad});
    ws_ = dmalloc<float>(ws_n * MB);
    ws_g_ = dmalloc<float>((size_t)std::max(kz_proj_ * d.joiner, kz_out_ * L_.vocab_pad) * MB);    // the search's own workspace: it runs beside encoder stages
    xin_ = dmalloc<float>(MB * d.embed_in);
    a3_ = dmalloc<float>(MB * d.f_out * L_.k3);
    HIP_CHECK(hipMemset(a3_, 0, MB * d.f_out * L_.k3 * 4));      // padded k columns (if any) stay zero
    // buffers that the front end / index fetch of flight k + 1 writes while flight k's layers or search still read them exist
    // once per flight parity (begin_flight() selects): encoder rows y + their sums of squares, the step's index arrays, the
    // round flags, the record offset, the batched encoder outputs (eout_lm_, allocated on first use)
    for (int p = 0; p < 2; ++p) { y_buf_[p] = dmalloc<float>(MB * d.d_model); ssq_buf_[p] = dmalloc<float>(MB * (d.d_model / SSQ_COLS)); }
    y_ = y_buf_[0]; ssq_ = ssq_buf_[0];
    ws_fe_ = dmalloc<float>((size_t)kz_embed_ * d.d_model * MB);      // the front end's own split-K planes (embed at small batches)
    ws_sr_ = dmalloc<float>((size_t)std::max(kz_proj_ * d.joiner, d.d_model) * MB);      // encoder_proj's, when it runs on the search stream
    // ... and the scratch rows of a macro step (u, xb, ff): a hosting layer graph runs problems of both parities in one launch ("ramp merge")
    for (int p = 0; p < 2; ++p) { xb_buf_[p] = dmalloc<float>(MB * d.d_model); u_buf_[p] = dmalloc<float>(MB * d.hidden); ff_buf_[p] = dmalloc<float>(MB * d.ffn); }
    xb_ = xb_buf_[0]; u_ = u_buf_[0]; ff_ = ff_buf_[0];
    ramp_mode_ = env_int("APRIL_RAMP_MERGE", 1);
    if (ramp_mode_ < 0 || ramp_mode_ > 3) ramp_mode_ = 1;
    ramp_d_ = dmalloc<RampState>(1); HIP_CHECK(hipMemset(ramp_d_, 0, sizeof(RampState)));
    if (ramp_mode_ == 1) {      // the latch's report: coherent pinned memory, the device stores to it and the host polls it
        HipLegacyLock legacy;
        HIP_CHECK(hipHostMalloc((void **)&ramp_word_h_, sizeof *ramp_word_h_, hipHostMallocCoherent)); *ramp_word_h_ = 0;
    }
    de_ = dmalloc<float>(MB * d.d_model);
    HIP_CHECK(hipMemset(de_, 0, MB * d.d_model * 4));            // rows whose context did not change are read (never stored) by the decoder projection
    logits_ = dmalloc<float>(3 * MB * d.vocab);
    logits_h_ = hmalloc<float>(3 * MB * d.vocab);
    // step bookkeeping
    // (two flights may be in the air -- the one the GPU runs and the one the host enqueues behind it -- so every per-flight
    // ring exists twice: flight parity p owns [p * cap, (p + 1) * cap) of the index blocks, step tables and records)
    ring_cap_ = std::max<size_t>((size_t)1 << 20, 3 * MB * 8 + 2 * S); ring_h_ = hmalloc<int>(2 * ring_cap_);
    step_cap_ = 1 << 14; step_off_h_ = hmalloc<int>((size_t)2 * step_cap_); rec_off_h_ = hmalloc<int>((size_t)2 * step_cap_);
    rec_cap_ = std::max<size_t>((size_t)1 << 20, 3 * MB * 8); rec_d_ = dmalloc<StepRecord>(2 * rec_cap_); rec_h_ = hmalloc<StepRecord>(2 * rec_cap_);
    for (int i = 0; i < 2; ++i) HIP_CHECK(hipEventCreateWithFlags(&flight_done_[i], hipEventDisableTiming));
    counter_d_ = dmalloc<int>(1);
    for (int p = 0; p < 2; ++p) {
        rec_off_buf_[p] = dmalloc<int>(1); flags_buf_[p] = dmalloc<int>(8); step_buf_[p] = dmalloc<int>(4 * MB);
        HIP_CHECK(hipMemset(rec_off_buf_[p], 0, 4)); HIP_CHECK(hipMemset(flags_buf_[p], 0, 32));
    }
    rec_off_d_ = rec_off_buf_[0]; flags_d_ = flags_buf_[0]; step_d_ = step_buf_[0];
    active_d_ = dmalloc<int>(MB); dirty_d_ = dmalloc<int>(MB);
    dec_slots_d_ = dmalloc<int>(std::max(S, MB));
    HIP_CHECK(hipMemset(counter_d_, 0, 4));

    upload_tables(ft);
    use_graphs_ = env_int("APRIL_NO_GRAPHS", 0) == 0;
    if (const int n = env_int("APRIL_GRAPH_CACHE_CAP", 0))        // tests: every family of captured chains is emptied early (a both-parity capture inserts two entries)
        step_graphs_.cap = lm_graphs_.cap = lm_search_graphs_.cap = sw_plan_cap_ = (size_t)std::max(n, 2), sw_graphs_.cap = 5 * sw_plan_cap_;
    free_.reserve(S);
    for (int i = cfg_.max_slots - 1; i >= 0; --i) free_.push_back(i);
    LOGI("engine: device %d, %d slots, max batch %d, weights %.1f MB, kz(embed,hr,ff2,proj,out)=%d,%d,%d,%d,%d",
         cfg_.device, cfg_.max_slots, cfg_.max_batch, L_.total * 4.0 / 1e6, kz_embed_, kz_hr_, kz_ff2_, kz_proj_, kz_out_);
}

void Engine::finish_weights()
{
    HipLegacyLock legacy;
    HIP_CHECK(hipSetDevice(cfg_.device));
    if (cfg_.precision == 1 && !wh_) {
        // fp16 operand mode (BASELINE configs[4]): every Linear / LSTM weight matrix gets an fp16 copy in the same
        // packed element order (round-to-nearest-even, on the device); convolutions, biases, embeddings stay fp32
        wh_ = dmalloc<uint16_t>(L_.total);
        for (const auto &sec : gemm_sections(L_)) launch_cvt_f16(w_ + sec.first, wh_ + sec.first, sec.second, nullptr);
        if (f16_tile_) {
            // the layer GEMMs once more, in the order of the 32-k MFMA's B fragment (the other GEMMs -- embed, encoder_proj,
            // decoder, joiner -- stay on the round-2 kernels and the copies above)
            const NetDims &d = L_.dims;
            wx_ = dmalloc<uint16_t>(L_.total);
            for (const PackedLayout::Layer &o : L_.layers) {
                launch_repack_x32(w_ + o.wg, wx_ + o.wg, 2 * d.d_model, 4 * d.hidden, nullptr);
                launch_repack_x32(w_ + o.whr, wx_ + o.whr, d.hidden, d.d_model, nullptr);
                launch_repack_x32(w_ + o.wff1, wx_ + o.wff1, d.d_model, d.ffn, nullptr);
                launch_repack_x32(w_ + o.wff2, wx_ + o.wff2, d.ffn, d.d_model, nullptr);
            }
        }
        HIP_CHECK(hipDeviceSynchronize());
    }
    if (!conv_wt_) {   // the many-chunk form of the conv front end reads its weights channel-fastest (kernels_misc.hip conv12_wide_kernel)
        const NetDims &d = L_.dims;
        conv_wt_ = dmalloc<float>((size_t)9 * d.conv_ch[0] + (size_t)9 * d.conv_ch[0] * d.conv_ch[1]);
        launch_conv_weight_transpose(w_ + L_.conv_w[0], w_ + L_.conv_w[1], d.conv_ch[0], d.conv_ch[1], conv_wt_, conv_wt_ + (size_t)9 * d.conv_ch[0], nullptr);
        HIP_CHECK(hipDeviceSynchronize());
    }
    build_dec_table();
}

// The decoder network is a pure function of the two context tokens (embedding, grouped conv over the context, ReLU, projection:
// reference src/april_session.c:151-163), so its output for EVERY context is computed once at load -- vocab^2 rows of `joiner`
// floats (500^2 x 512 x 4 B = 512 MB of this GPU's 288 GB) by the same kernels that would run per emitted token -- and the
// joiner reads the row of a session's current context.  A context change then costs nothing: no decoder launches in the chunk
// chain (2..3 per search round), none at session start or after a flush.  Not built for context != 2 or when the table would
// exceed APRIL_DEC_TABLE_MB (default 2048; 0 disables): those models run the decoder per context change as before.
void Engine::build_dec_table()
{
    if (dec_table_) return;
    const NetDims &d = L_.dims;
    const size_t limit_mb = (size_t)std::max(0, env_int("APRIL_DEC_TABLE_MB", 2048));
    const size_t rows = (size_t)d.vocab * (size_t)d.vocab;
    if (d.context != 2 || rows * (size_t)d.joiner * 4 > limit_mb * 1024 * 1024 || rows * (size_t)d.joiner * 4 >= ((size_t)1 << 32)) return;   // (32-bit byte offsets in the GEMM's A addressing)
    const int MB = cfg_.max_batch;
    float *table = dmalloc<float>(rows * (size_t)d.joiner);
    std::vector<int> iota((size_t)MB), ctx((size_t)MB * 2);
    for (int i = 0; i < MB; ++i) iota[(size_t)i] = i;
    int *ctx_d = dmalloc<int>((size_t)MB * 2);
    HIP_CHECK(hipMemcpy(dec_slots_d_, iota.data(), (size_t)MB * 4, hipMemcpyHostToDevice));
    for (size_t base = 0; base < rows; base += (size_t)MB) {
        const int n = (int)std::min<size_t>((size_t)MB, rows - base);
        for (int i = 0; i < n; ++i) { const size_t r = base + (size_t)i; ctx[(size_t)2 * i] = (int)(r / (size_t)d.vocab); ctx[(size_t)2 * i + 1] = (int)(r % (size_t)d.vocab); }
        HIP_CHECK(hipMemcpy(ctx_d, ctx.data(), (size_t)n * 8, hipMemcpyHostToDevice));
        DecEmbedArgs a; a.dec = dec_params(); a.ctx = ctx_d; a.M = n; a.out = de_; a.ldo = d.d_model;
        launch_dec_embed(a, stream_);
        run_decproj(n, dec_slots_d_, nullptr, nullptr, 1, table + base * (size_t)d.joiner);
        HIP_CHECK(hipStreamSynchronize(stream_));
    }
    (void)hipFree(ctx_d);
    dec_table_ = table;
    LOGI("engine: decoder table %zu rows x %d (%.0f MB)", rows, d.joiner, rows * (double)d.joiner * 4 / 1e6);
}

Engine::~Engine()
{
    HipLegacyLock legacy;
    (void)hipSetDevice(cfg_.device);
    settle_pending_layers(true, RampDefer::BY_OTHER);      // (a deferred layer graph, its search and its flight event: enqueued, then waited for like the rest)
    (void)hipStreamSynchronize(f_stream_); (void)hipStreamSynchronize(stream_); (void)hipStreamSynchronize(s_stream_);
    dump_stream_trace();
    if (ramp_d_ && ramp_eligible_.load() > 0) {
        unsigned h = 0;
        if (hipMemcpy(&h, &ramp_d_->hosted, sizeof h, hipMemcpyDeviceToHost) == hipSuccess) LOGI("engine: ramp merge: %u of %llu hostable split feeds were hosted by their predecessor", h, (unsigned long long)ramp_eligible_.load());
        if (defer_.deferred) LOGI("engine: ramp merge: %llu layer graphs deferred, %llu launched headless; settled by the flight wait %llu, by another entry %llu", (unsigned long long)defer_.deferred,
                                  (unsigned long long)defer_.headless, (unsigned long long)defer_.settled_by[RampDefer::BY_WAIT], (unsigned long long)defer_.settled_by[RampDefer::BY_OTHER]);
    }
    for (StreamTrace &t : trace_) for (hipEvent_t e : t.ev) if (e) (void)hipEventDestroy(e);
    if (trace_base_) (void)hipEventDestroy(trace_base_);
    for (hipEvent_t e : join_ev_) (void)hipEventDestroy(e);
    for (auto &e : ev_pool_) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    drop_graphs(); free_sw_plans(); if (gclk_slots_) (void)hipFree(gclk_slots_);
    if (lm_stream_) { (void)hipStreamSynchronize(lm_stream_); (void)hipStreamDestroy(lm_stream_); }
    for (hipEvent_t e : lm_events_) (void)hipEventDestroy(e);
    if (zargs_h_) { (void)hipHostFree(zargs_h_); (void)hipFree(zargs_d_); }
    for (int i = 0; i < 3; ++i) if (zargs_done_[i]) (void)hipEventDestroy(zargs_done_[i]);
    for (void *p : {(void *)lm_now_d_, (void *)lm_rows_d_, (void *)lm_rec_off_d_}) if (p) (void)hipFree(p);
    conf_k_.release(); bias_set_.release(); bias_desc_.release(); opt_.release();
    if (conf_d_) (void)hipFree(conf_d_);
    if (conf_h_) (void)hipHostFree(conf_h_);
    for (auto &b : bias_sets_) if (b.dev) (void)hipFree(b.dev);
    if (bias_state_d_) (void)hipFree(bias_state_d_);
    lm_slot_.release(); lm_desc_.release();
    for (auto &e : lm_models_) if (e.dev) (void)hipFree(e.dev);
    if (lm_state_d_) (void)hipFree(lm_state_d_);
    for (void *p : {(void *)vad_state_d_, (void *)pass_out_d_}) if (p) (void)hipFree(p);
    for (PassBlock &k : pass_blocks_) (void)hipHostFree(k.h);
    if (snap_d_) (void)hipFree(snap_d_);
    if (snap_h_) (void)hipHostFree(snap_h_);
    if (ws_g_) (void)hipFree(ws_g_);
    if (conv_wt_) (void)hipFree(conv_wt_);
    if (dec_table_) (void)hipFree(dec_table_);
    if (p_lm_) (void)hipFree(p_lm_);
    for (int p = 0; p < 2; ++p)
        for (void *q : {(void *)eout_lm_buf_[p], (void *)y16_buf_[p], (void *)y_buf_[p], (void *)ssq_buf_[p], (void *)xb_buf_[p], (void *)u_buf_[p], (void *)ff_buf_[p],
                        (void *)xb16_buf_[p], (void *)u16_buf_[p], (void *)ff16_buf_[p], (void *)rec_off_buf_[p], (void *)flags_buf_[p], (void *)step_buf_[p]}) if (q) (void)hipFree(q);
    if (ws_fe_) (void)hipFree(ws_fe_);
    if (ws_sr_) (void)hipFree(ws_sr_);
    if (ramp_word_h_) (void)hipHostFree(ramp_word_h_);
    for (void *p : {(void *)wx_, (void *)h16_, (void *)ramp_d_}) if (p) (void)hipFree(p);      // (fp16 tile path; ramp merge)
    for (void *p : {(void *)w_, (void *)wh_, (void *)h_, (void *)c_, (void *)ring_, (void *)eout_, (void *)dout_, (void *)gstate_, (void *)cls_, (void *)ws_, (void *)xin_,
                    (void *)a3_, (void *)de_, (void *)logits_, (void *)rec_d_, (void *)counter_d_,
                    (void *)active_d_, (void *)dirty_d_, (void *)dec_slots_d_,
                    (void *)ds_pcm_[0], (void *)ds_pcm_[1]})
        if (p) (void)hipFree(p);
    for (void *p : {(void *)ring_h_, (void *)step_off_h_, (void *)rec_off_h_, (void *)rec_h_, (void *)logits_h_, (void *)hs_pcm_[0], (void *)hs_pcm_[1]})
        if (p) (void)hipHostFree(p);
    for (int b = 0; b < 2; ++b) if (fb_done_[b]) (void)hipEventDestroy(fb_done_[b]);
    for (int b = 0; b < 2; ++b) if (flight_done_[b]) (void)hipEventDestroy(flight_done_[b]);
    for (void *p : table_allocs_) (void)hipFree(p);
    (void)hipStreamDestroy(stream_); (void)hipStreamDestroy(f_stream_); (void)hipStreamDestroy(s_stream_);
}

void Engine::upload_tables(const FbankHostTables &ft)
{
    auto up = [&](const void *src, size_t bytes) {
        void *p = nullptr;
        HIP_CHECK(hipMalloc(&p, std::max<size_t>(bytes, 16)));
        if (bytes) HIP_CHECK(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
        table_allocs_.push_back(p);
        return p;
    };
    ft_.window = (const float *)up(ft.window.data(), ft.window.size() * 4);
    ft_.mel = (const float *)up(ft.mel.data(), ft.mel.size() * 4);
    ft_.mel_lo = (const int *)up(ft.mel_lo.data(), ft.mel_lo.size() * 4);
    ft_.mel_hi = (const int *)up(ft.mel_hi.data(), ft.mel_hi.size() * 4);
    ft_.nfct = (int)ft.factors.size();
    for (int k = 0; k < ft_.nfct; ++k) {
        ft_.fct[k] = ft.factors[(size_t)k];
        ft_.tw[k] = (const double *)up(ft.tw[(size_t)k].data(), ft.tw[(size_t)k].size() * 8);
        ft_.tws[k] = ft.tws[(size_t)k].empty() ? nullptr : (const double *)up(ft.tws[(size_t)k].data(), ft.tws[(size_t)k].size() * 8);
    }
    ft_.padded = ft.padded; ft_.nbins = ft.nbins;
    pad_value_ = ft.pad_value;
}

int Engine::alloc_slot()
{
    std::lock_guard<std::mutex> g(slot_mu_);
    if (free_.empty() && !zero_pending_.empty()) zero_pending_slots();
    if (free_.empty()) return -1;
    const int s = free_.back();
    free_.pop_back();
    ++live_;
    return s;
}

// (slot_mu_ held) reset every slot that was freed since the last call: up to 64 slots per launch instead of one launch per
// aas_free -- tearing down 2048 sessions cost 2048 launches (4.3 ms of the stream, profiles/r03_b2048_kernel_stats.csv)
void Engine::zero_pending_slots()
{
    if (zero_pending_.empty()) return;
    // Teardown-tolerant: sessions may be freed while the process is exiting and the HIP runtime is already gone.
    if (hipSetDevice(cfg_.device) == hipSuccess) {
        std::lock_guard<std::mutex> cg(capture_mu_);           // never enqueue into a stream that is being captured (step())
        m_touched();
        const NetDims &d = L_.dims;
        for (size_t o = 0; o < zero_pending_.size(); o += 64) {
            ZeroSlotArgs z;
            z.h = h_; z.c = c_; z.n_layers = d.n_layers; z.slots = (size_t)cfg_.max_slots; z.d_model = d.d_model; z.hidden = d.hidden;
            z.eout = eout_; z.dout = dout_; z.joiner = d.joiner; z.state = gstate_; z.blank = P_.blank_id; z.h16 = h16_;
            z.n_list = (int)std::min<size_t>(64, zero_pending_.size() - o);
            for (int i = 0; i < z.n_list; ++i) z.list[i] = zero_pending_[o + (size_t)i];
            launch_zero_slot(z, stream_);
        }
    }
    for (int s : zero_pending_) free_.push_back(s);
    zero_pending_.clear();
}

void Engine::free_slot(int slot)
{
    // the slot goes back to the free list once it has been reset to the reference's calloc'd tensors (april_session.c:40-58)
    // and a [blank, blank] context -- in a batch: when 256 freed slots have gathered, when the free list runs dry, or before
    // the next flight is launched (begin_flight), stream-ordered ahead of any later use of the slot
    // the next owner starts with confidences off, without a bias set (at the root) and without search options (dropped at the push while nothing was ever on)
    set_slot_confidence(slot, 0); set_slot_bias(slot, nullptr); set_slot_lm(slot, nullptr, 0.0f, 0.0f); set_slot_search_options(slot, SearchOpt{0u, 0.0f});
    std::lock_guard<std::mutex> g(slot_mu_);
    zero_pending_.push_back(slot);
    --live_;
    if (zero_pending_.size() >= 256) zero_pending_slots();
}

// Waits for the three streams and touches nothing else: safe from any thread (the readers below are called by client threads
// while the stepping thread keeps enqueueing).
void Engine::sync_streams()
{
    settle_pending_layers(true, RampDefer::BY_OTHER);      // (what is deferred belongs to "everything enqueued so far")
    HIP_CHECK(hipStreamSynchronize(f_stream_)); HIP_CHECK(hipStreamSynchronize(stream_)); HIP_CHECK(hipStreamSynchronize(s_stream_));
}

// Stepping thread only (or under capture_mu_): everything enqueued so far is done, so no stream has work another one has not seen.
// A client thread must NOT clear these flags -- between its stream waits and the store the stepping thread may have enqueued a new
// fbank and set one; it uses sync_streams(), a stale "unseen" only costs a redundant event.
void Engine::sync()
{
    m_touched();
    sync_streams();
    f_unseen_by_m_ = s_unseen_by_m_ = m_unseen_by_f_ = m_unseen_by_s_ = false;
    if (profiling_) collect_timing();
}

// Graph captures use hipStreamCaptureModeRelaxed AND hold hip_legacy_mutex() (engine.h): a capture begun in the thread-local (or
// global) mode makes every "potentially unsafe" HIP call -- hipMalloc, hipMemcpy, hipFree ... -- of every OTHER thread that is in the
// default global mode fail with hipErrorStreamCaptureUnsupported for as long as the capture lasts; in relaxed mode a legacy-stream copy
// of another thread still fails ("would make the legacy stream depend on a capturing blocking stream", although the streams here are
// non-blocking) and invalidates the capture.  Client threads make exactly such calls: another model being loaded,
// aprilx_session_read_frames / aprilx_session_context on an idle session while other sessions stream (found in round 5 by running
// tests/sched_harness/driver.cc against the real engine: the reader's hipMemcpy aborted the process).  The stepping thread itself
// issues nothing but kernel launches, async copies and event records inside a capture.
template <typename Chain> static hipGraphExec_t capture_graph(hipStream_t st, Chain &&chain)
{
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    HipLegacyLock capture_guard;      // (no legacy-stream call of any thread during the capture: see engine.h)
    HIP_CHECK(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
    chain();
    HIP_CHECK(hipStreamEndCapture(st, &graph));
    HIP_CHECK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    HIP_CHECK(hipGraphDestroy(graph));
    return exec;
}

void GraphCache::clear()
{
    if (!map_.empty()) LOGI("engine: %s graphs emptied (%zu entries)", name, map_.size());
    for (auto &g : map_) (void)hipGraphExecDestroy(g.second);
    map_.clear(); uses_.clear();
}

// the family's graph for `key`, captured now when it is missing (the caller has made room)
template <typename Chain> hipGraphExec_t Engine::cached_graph(GraphCache &cache, const GraphCache::Key &key, hipStream_t st, Chain &&chain)
{
    if (!cache.find(key)) cache.insert(key, capture_graph(st, chain));
    return cache.find(key);
}

// A chain that is captured at its second use is captured for BOTH flight parities (the parity selects buffers): which parity a shape meets depends
// on the history of flights (feeds alternate between 2 and 3 chunks, parities alternate too, one merged or empty flight flips the pairing), and a capture in
// mid-stream is a 3 ms hiccup.  `capture` runs once per parity and fills the cache (cached_graph): the other parity first, this one last, so the member pointers end where they were.
template <typename Capture> void Engine::capture_both_parities(Capture &&capture)
{
    const int par = flight_parity_;
    m_touched();
    for (int q : {1 - par, par}) { select_parity(q); capture(); }
}

// ---------------------------------------------------------------- streams
// Three in-order streams.  stream_ (M) carries the layer chain and every launch of the general paths; f_stream_ (F) the PCM
// upload and the fbank kernel of every flight and, for a feed that runs as a split wavefront (lm_step mode 1), its index fetch
// and conv / embed front end; s_stream_ (S) the search of such a feed.  Inside one flight FE -> layers -> search are chained by
// events; ACROSS flights the front end of flight k + 1 and the search of flight k run beside the layers of flights k / k + 1
// (they share no buffer: see the per-parity buffers in the constructor).  The general paths (chunk-by-chunk steps, long feeds,
// decoder refreshes, traced steps) stay on M and first wait for whatever F and S still have in the air; a split feed after
// general work makes F and S wait for M the same way.  The flags say which stream has work the other has not waited for yet.
// APRIL_STREAM_TRACE=<file> (measurement): hipEvent time stamps around the three parts of every split feed -- front end on F,
// layers on M, search on S -- written as one line per feed when the engine is destroyed: the evidence that neighbouring feeds'
// parts overlap (rocprofv3's kernel trace serialises the queues, so it cannot show it).
Engine::StreamTrace *Engine::trace_slot()
{
    static const char *path = env_str("APRIL_STREAM_TRACE");
    if (!path) return nullptr;
    if (!trace_base_) { HIP_CHECK(hipEventCreate(&trace_base_)); HIP_CHECK(hipEventRecord(trace_base_, stream_)); }
    if (trace_.size() >= 4096) return nullptr;
    trace_.emplace_back();
    StreamTrace &t = trace_.back();
    for (hipEvent_t &e : t.ev) HIP_CHECK(hipEventCreate(&e));
    return &t;
}

void Engine::dump_stream_trace()
{
    const char *path = env_str("APRIL_STREAM_TRACE");
    if (!path || trace_.empty()) return;
    FILE *f = fopen(path, "w");
    if (!f) return;
    fprintf(f, "# one line per split feed; times in us since the first split feed; FE = index fetch + conv + embed on stream F, LY = layer wavefront on M, SR = encoder_proj + search on S\n");
    fprintf(f, "# feed sessions chunks  FE_start FE_end  LY_start LY_end  SR_start SR_end   overlap: FE inside the previous feed's LY window? SR inside the next feed's LY window?  LY flavour: headless / head\n");
    std::vector<std::array<float, 6>> ts;
    for (StreamTrace &t : trace_) {
        std::array<float, 6> a{};
        bool ok = t.used;
        for (int i = 0; i < 6 && ok; ++i) ok = hipEventElapsedTime(&a[(size_t)i], trace_base_, t.ev[i]) == hipSuccess;
        if (ok) ts.push_back(a); else (void)hipGetLastError();
    }
    for (size_t i = 0; i < ts.size(); ++i) {
        const auto &a = ts[i];
        const bool fe_in_prev = i > 0 && a[0] * 1e3f < ts[i - 1][3] * 1e3f && a[1] * 1e3f > ts[i - 1][2] * 1e3f;
        const bool sr_in_next = i + 1 < ts.size() && a[5] > ts[i + 1][2] && a[4] < ts[i + 1][3];
        fprintf(f, "%4zu %5d %2d  %10.1f %10.1f  %10.1f %10.1f  %10.1f %10.1f   %s %s %s\n", i, trace_[i].m, trace_[i].T, a[0] * 1e3, a[1] * 1e3, a[2] * 1e3, a[3] * 1e3, a[4] * 1e3, a[5] * 1e3,
                fe_in_prev ? "FE<prevLY" : "-", sr_in_next ? "SR<nextLY" : "-", trace_[i].headless ? "headless" : "head");
    }
    fclose(f);
}

void Engine::join(hipStream_t waiter, hipStream_t src)
{
    hipEvent_t e = join_ev_[join_pos_++ % join_ev_.size()];
    HIP_CHECK(hipEventRecord(e, src));
    HIP_CHECK(hipStreamWaitEvent(waiter, e, 0));
}

void Engine::general_prologue()
{
    m_touched();
    if (f_unseen_by_m_) { join(stream_, f_stream_); f_unseen_by_m_ = false; }
    if (s_unseen_by_m_) { join(stream_, s_stream_); s_unseen_by_m_ = false; }
    m_unseen_by_f_ = m_unseen_by_s_ = true;
    flight_tail_s_ = false;
}

// ---------------------------------------------------------------- profiling
void Engine::set_profiling(bool on) { std::lock_guard<std::mutex> cg(capture_mu_); sync(); profiling_ = on; }
void Engine::reset_timing() { for (auto &t : timing_) t = KernelTiming(); }
void Engine::set_gates_clock(bool on)
{
    std::lock_guard<std::mutex> cg(capture_mu_);
    HIP_CHECK(hipSetDevice(cfg_.device));
    sync();
    if (on) {
        if (!gclk_slots_) gclk_slots_ = dmalloc<unsigned long long>((size_t)GCLK_SLOTS * STAMP_WORDS);
        HIP_CHECK(hipMemsetAsync(gclk_slots_, 0, (size_t)GCLK_SLOTS * STAMP_WORDS * 8, stream_));
        HIP_CHECK(hipStreamSynchronize(stream_));
        gclk_ms_ = 0; gclk_launches_ = 0; gclk_rows_ = 0;
        for (int i = 0; i < 4; ++i) { gclk_ms_n_[i] = 0; gclk_launches_n_[i] = 0; }
        gclk_ = true;
        return;
    }
    collect_gates_clock(); gclk_ = false;
}
// every plan built while the clock was on: its slots' sums (10 ns ticks of s_memrealtime) and launch counts (clock switched off; plans about to be discarded)
void Engine::collect_gates_clock()
{
    if (!gclk_ || !gclk_slots_) return;
    std::vector<unsigned long long> h((size_t)GCLK_SLOTS * STAMP_WORDS);
    HIP_CHECK(hipMemcpyAsync(h.data(), gclk_slots_, h.size() * 8, hipMemcpyDeviceToHost, stream_)); HIP_CHECK(hipStreamSynchronize(stream_));
    for (auto &kv : sw_plans_)
        for (size_t i = 0; i < kv.second.stamp_slots.size(); ++i) {
            const auto &sl = kv.second.stamp_slots[i];
            const unsigned long long ticks = h[(size_t)sl.first * STAMP_WORDS + 2], n = h[(size_t)sl.first * STAMP_WORDS + 3];
            gclk_ms_ += (double)ticks * 1e-5; gclk_launches_ += (long)n; gclk_rows_ += (long)n * sl.second;
            const int bn = std::min(std::max(kv.second.stamp_n[i], 1), 4) - 1;
            gclk_ms_n_[bn] += (double)ticks * 1e-5; gclk_launches_n_[bn] += (long)n;
        }
}
void Engine::timed_begin(int cls)
{
    ++launch_count_;
    if (!profiling_) return;
    if (ev_used_ == ev_pool_.size()) { Ev e; HIP_CHECK(hipEventCreate(&e.a)); HIP_CHECK(hipEventCreate(&e.b)); e.cls = cls; ev_pool_.push_back(e); }
    ev_pool_[ev_used_].cls = cls;
    // gates launches: the kernel's own dispatch time stamps (hipExtLaunchKernel through APRIL_LAUNCH) instead of event packets around
    // it -- the clock of rocprofv3's per-kernel duration, which bench.py's roofline is priced on; other classes: brackets on the stream
    if (cls == T_GATES) gemm_profile_next_launch(ev_pool_[ev_used_].a, ev_pool_[ev_used_].b);
    else HIP_CHECK(hipEventRecord(ev_pool_[ev_used_].a, stream_));
}
void Engine::timed_end(int cls)
{
    if (!profiling_) return;
    if (cls == T_GATES) {
        // (every GEMM launcher goes through APRIL_LAUNCH, which consumes the pair; a guard for a launch path that does not: drop the sample instead of reading unrecorded events)
        if (gemm_profile_pending()) { gemm_profile_next_launch(nullptr, nullptr); return; }
    } else HIP_CHECK(hipEventRecord(ev_pool_[ev_used_].b, stream_));
    ++ev_used_;
}
void Engine::collect_timing()
{
    for (size_t i = 0; i < ev_used_; ++i) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev_pool_[i].a, ev_pool_[i].b) == hipSuccess) { timing_[ev_pool_[i].cls].ms += ms; timing_[ev_pool_[i].cls].launches++; }
    }
    ev_used_ = 0;
}

// ---------------------------------------------------------------- fbank
// bytes per descriptor of the staged arrays; the observers' arrays follow the block's order (staging_layout.h, pass_layout.h)
static_assert(ST_VD + OBS_DTMF == ST_DT && ST_VD + OBS_TONE == ST_TN && ST_VD + OBS_QUALITY == ST_QA && ST_VD + OBS_COUNT == ST_COUNT, "observer o stages array ST_VD + o");
static const StagingSizes kStagingEl = [] {
    StagingSizes el{};
    el[ST_FRAMES] = sizeof(FbankFrameDesc); el[ST_RS] = sizeof(ResampleDesc); el[ST_DC] = sizeof(DecodeDesc);
    el[ST_VD] = sizeof(VadDesc); el[ST_DT] = sizeof(DtmfDesc); el[ST_TN] = sizeof(ToneDesc); el[ST_QA] = sizeof(QualityDesc);
    return el;
}();

const uint8_t *Engine::fbank(int n_frames, const FbankFrameDesc *desc, const std::pair<const int16_t *, size_t> *parts, size_t n_parts, size_t n_pcm, HostPool *pool,
                             const FrontPass &pass)
{
    if (n_frames <= 0) return nullptr;
    const int n_rs = std::max(pass.n_rs, 0), n_dc = std::max(pass.n_dc, 0);
    ResampleDesc *rs = pass.rs;
    const DecodeDesc *dc = pass.dc;
    const size_t n_in_parts = n_rs ? pass.n_in_parts : 0, n_raw_parts = n_dc ? pass.n_raw_parts : 0;
    // the observers: descriptors and frames per observer, and where their records go (pass_layout.h)
    int n_obs[OBS_COUNT]; PassFrames obs_frames; bool observed = false;
    for (int o = 0; o < OBS_COUNT; ++o) {
        n_obs[o] = std::max(pass.obs[o].n, 0); obs_frames[(size_t)o] = n_obs[o] ? pass.obs[o].frames : 0;
        observed = observed || n_obs[o];
    }
    const int n_vd = n_obs[OBS_VAD], n_dt = n_obs[OBS_DTMF], n_tn = n_obs[OBS_TONE], n_qa = n_obs[OBS_QUALITY];
    const PassLayout out = pass_layout(obs_frames);
    StagingCounts cnt;
    cnt.n_pcm = n_pcm; cnt.n_in = n_rs ? pass.n_in : 0; cnt.n_raw = n_dc ? pass.n_raw : 0;
    cnt.n[ST_FRAMES] = (size_t)n_frames; cnt.n[ST_RS] = (size_t)n_rs; cnt.n[ST_DC] = (size_t)n_dc;
    for (int o = 0; o < OBS_COUNT; ++o) cnt.n[(size_t)(ST_VD + o)] = (size_t)n_obs[o];
    const StagingLayout lay = staging_layout(cnt, kStagingEl);
    HIP_CHECK(hipSetDevice(cfg_.device));
    for (int i = 0; i < n_rs; ++i) rs[i].taps = resample_table(pass.rs_specs[i]);      // (uploaded at a conversion's first use)
    if (!fb_caps_.holds(cnt, lay)) {
        sync();
        HipLegacyLock regrow_guard;                   // (frees imply a device synchronisation: not beside another engine's capture; order: capture_mu_, then this)
        for (int b = 0; b < 2; ++b) if (hs_pcm_[b]) { (void)hipHostFree(hs_pcm_[b]); (void)hipFree(ds_pcm_[b]); }
        fb_caps_.grow(cnt, lay);
        const size_t units = fb_caps_.units(kStagingEl);
        for (int b = 0; b < 2; ++b) {
            hs_pcm_[b] = hmalloc<int16_t>(units); ds_pcm_[b] = dmalloc<int16_t>(units);
            if (!fb_done_[b]) HIP_CHECK(hipEventCreateWithFlags(&fb_done_[b], hipEventDisableTiming));
        }
    }
    PassBlock *block = nullptr;
    const float *dt_tables = n_dt ? dtmf_tables() : nullptr;      // (sets dt_wd_)
    const float *tn_tables = n_tn ? tone_tables() : nullptr;      // (sets tn_w_, tn_f_)
    if (observed) {
        // a pass with observers' descriptors: the first VAD pass of the engine allocates the per-slot records; the device's block grows
        // behind a sync (earlier passes' copies read it); a pass takes a pinned block nobody holds, or a new one (warm-up only)
        if (n_vd && !vad_state_d_) vad_state_d_ = dmalloc<VadState>((size_t)cfg_.max_slots);
        if (out.bytes > pass_out_cap_) {
            sync();
            HipLegacyLock guard;
            if (pass_out_d_) (void)hipFree(pass_out_d_);
            pass_out_cap_ = std::max<size_t>(out.bytes * 2, 4096);
            pass_out_d_ = dmalloc<uint8_t>(pass_out_cap_);
        }
        for (PassBlock &k : pass_blocks_) if (!k.busy && k.cap >= out.bytes && (!block || k.cap < block->cap)) block = &k;
        if (!block) {
            PassBlock k;
            k.cap = 4096; while (k.cap < out.bytes) k.cap *= 2;
            k.h = hmalloc<uint8_t>(k.cap);
            pass_blocks_.push_back(k);
            block = &pass_blocks_.back();
        }
        block->busy = true;
    }
    const int b = fb_flip_;
    fb_flip_ ^= 1;
    HIP_CHECK(hipEventSynchronize(fb_done_[b]));          // the launch that used this pair two calls ago has consumed it
    const size_t woff = lay.raw, doff = lay.off[ST_FRAMES], roff = lay.off[ST_RS], coff = lay.off[ST_DC], voff = lay.off[ST_VD], bytes = lay.bytes;      // (staging_layout.h)
    char *hs = reinterpret_cast<char *>(hs_pcm_[b]);
    const char *dev = reinterpret_cast<const char *>(ds_pcm_[b]);
    memcpy(hs + doff, desc, (size_t)n_frames * sizeof(FbankFrameDesc));
    if (n_vd) memcpy(hs + voff, pass.descs<VadDesc>(), (size_t)n_vd * sizeof(VadDesc));
    // The runs of an observer that reads staged samples (DTMF, tones, line quality): its descriptors go into the staging buffer; every run
    // lies inside the frames of this call and inside the observer's part of the block, `ok` holds for it and no padding row is among its
    // frames (else abort); then what the observers' args share -- samples, frame descriptors, descriptors, max_n, the part of the block
    auto stage_runs = [&](auto &a, const char *what, auto ok) {
        typedef std::remove_cv_t<std::remove_pointer_t<decltype(a.desc)>> Desc;
        const Observer o = FrontPass::observer_of(a.desc);
        const Desc *runs = pass.descs<Desc>();
        const size_t at = lay.off[(size_t)(ST_VD + o)];
        memcpy(hs + at, runs, (size_t)n_obs[o] * sizeof(Desc));
        for (int i = 0; i < n_obs[o]; ++i) {
            const Desc &t = runs[i];
            if (t.n <= 0 || t.first < 0 || t.first + t.n > n_frames || t.out_off < 0 || (size_t)t.out_off + (size_t)t.n > obs_frames[(size_t)o] || !ok(t)) {
                LOGE("fbank: %s descriptor %d outside the pass", what, i); abort();
            }
            for (int k = 0; k < t.n; ++k) if (desc[t.first + k].pcm_off < 0) { LOGE("fbank: a padding row inside %s run %d", what, i); abort(); }
            a.max_n = std::max(a.max_n, t.n);
        }
        a.pcm = ds_pcm_[b]; a.frames = reinterpret_cast<const FbankFrameDesc *>(dev + doff);
        a.desc = reinterpret_cast<const Desc *>(dev + at); a.n_desc = n_obs[o];
        a.out = reinterpret_cast<decltype(a.out)>(pass_out_d_ + out.at[o]);
    };
    DtmfArgs ta;
    if (n_dt) { stage_runs(ta, "DTMF", [&](const DtmfDesc &t) { return t.plan.Wd == dt_wd_; }); ta.tables = dt_tables; ta.wd = dt_wd_; }
    ToneArgs na;
    if (n_tn) { stage_runs(na, "tone", [&](const ToneDesc &t) { return t.plan.W == tn_w_ && t.plan.F == tn_f_; }); na.tables = tn_tables; na.w = tn_w_; na.f = tn_f_; }
    QualityArgs qa;
    if (n_qa) {
        if (pass.quality_hop <= 0 || pass.quality_hop > ft_.padded) { LOGE("fbank: a quality hop of %d samples is not inside the frame", pass.quality_hop); abort(); }
        stage_runs(qa, "quality", [](const QualityDesc &) { return true; });
        qa.hop = pass.quality_hop;
    }
    ResampleArgs ra;
    if (n_rs) {
        ResampleDesc *hr = reinterpret_cast<ResampleDesc *>(hs + roff);
        int64_t blocks = 0, lds = 0;
        for (int i = 0; i < n_rs; ++i) {
            hr[i] = rs[i];
            hr[i].in_off += (int32_t)n_pcm;
            blocks = std::max<int64_t>(blocks, (rs[i].out_cnt + kResampleBlock - 1) / kResampleBlock);
            lds = std::max<int64_t>(lds, resample_lds_floats(rs[i].L, rs[i].M, rs[i].K));
        }
        ra.n_desc = n_rs; ra.max_blocks = (int)blocks; ra.lds_floats = (int)lds;
    }
    DecodeArgs da;
    if (n_dc) {
        DecodeDesc *hd = reinterpret_cast<DecodeDesc *>(hs + coff);
        int64_t blocks = 0; uint64_t frames = 0;
        for (int i = 0; i < n_dc; ++i) {
            hd[i] = dc[i];
            if (dc[i].dst_in) hd[i].dst += (int32_t)n_pcm;
            blocks = std::max<int64_t>(blocks, (dc[i].out_cnt + kDecodeBlock - 1) / kDecodeBlock);
            frames += (uint64_t)dc[i].n_src;
        }
        da.n_desc = n_dc; da.max_blocks = (int)blocks;
        dc_launches_.fetch_add(1, std::memory_order_relaxed); dc_frames_.fetch_add(frames, std::memory_order_relaxed);
    }
    // the PCM: windows of default sessions are copied, the model-rate regions of resampled windows only reserved (null pointer);
    // `base` is the parts' first element in the staging buffer, parts and base in units of the parts' own element (int16, raw byte)
    auto stage = [&](const auto *pp, size_t np, size_t base) {
        const size_t el = sizeof(*pp[0].first);
        char *dst = hs;
        if (pool && np >= 256) {
            part_off_.resize(np);
            size_t off = base;
            for (size_t i = 0; i < np; ++i) { part_off_[i] = off; off += pp[i].second; }
            pool->run(np, 64, [&](size_t i) { if (pp[i].first) memcpy(dst + part_off_[i] * el, pp[i].first, pp[i].second * el); });
        } else {
            size_t off = base;
            for (size_t i = 0; i < np; ++i) { if (pp[i].first) memcpy(dst + off * el, pp[i].first, pp[i].second * el); off += pp[i].second; }
        }
    };
    stage(parts, n_parts, 0);
    if (n_in_parts) stage(pass.in_parts, n_in_parts, n_pcm);
    if (n_raw_parts) stage(pass.raw_parts, n_raw_parts, woff);
    std::lock_guard<std::mutex> cg(capture_mu_);
    if (m_unseen_by_f_) { join(f_stream_, stream_); m_unseen_by_f_ = false; }      // (general-path work may still read ring rows this call overwrites)
    HIP_CHECK(hipMemcpyAsync(ds_pcm_[b], hs_pcm_[b], bytes, hipMemcpyHostToDevice, f_stream_));
    FbankArgs a;
    a.t = ft_; a.pcm = ds_pcm_[b]; a.desc = reinterpret_cast<const FbankFrameDesc *>(dev + doff); a.n_frames = n_frames; a.ring = ring_; a.ring_frames = ring_frames_; a.pad_value = pad_value_;
    if (n_rs) { ra.in = ds_pcm_[b]; ra.out = ds_pcm_[b]; ra.desc = reinterpret_cast<const ResampleDesc *>(dev + roff); }
    if (n_dc) {
        da.raw = reinterpret_cast<const uint8_t *>(ds_pcm_[b]) + woff; da.out = ds_pcm_[b];
        da.desc = reinterpret_cast<const DecodeDesc *>(dev + coff);
    }
    VadArgs va;
    if (n_vd) {
        va.ring = ring_; va.ring_frames = ring_frames_; va.nbins = ft_.nbins; va.state = vad_state_d_; va.out = pass_out_d_ + out.at[OBS_VAD];
        va.desc = reinterpret_cast<const VadDesc *>(dev + voff); va.n_desc = n_vd;
    }
    // The launches, in stream order.  A profiled pass runs on M, behind its upload, each launch between the hipEvents of its class (they live on M).
    const bool timed = profiling_;
    const hipStream_t st = timed ? stream_ : f_stream_;
    if (timed) { m_touched(); join(stream_, f_stream_); }
    auto run = [&](int cls, auto launch) { if (timed) timed_begin(cls); launch(); if (timed) timed_end(cls); };
    if (n_dc) run(T_DECODE, [&] { launch_decode(da, st); });            // (decode feeds both)
    if (n_rs) run(T_RESAMPLE, [&] { launch_resample(ra, st); });
    if (n_dt) run(T_DTMF, [&] { launch_dtmf(ta, st); });                // (reads the samples fbank_kernel reads; the staging pair is recycled after fb_done_)
    if (n_tn) run(T_TONE, [&] { launch_tone(na, st); });                // (likewise)
    if (n_qa) run(T_QUALITY, [&] { launch_quality(qa, st); });          // (likewise)
    run(T_FBANK, [&] { launch_fbank(a, st); });
    if (n_vd) run(T_VAD, [&] { launch_vad(va, st); });
    if (timed) join(f_stream_, stream_);
    if (observed) {       // the pass's block -> its pinned block, in front of fb_done_; read after the flight's wait (close_flight)
        HIP_CHECK(hipMemcpyAsync(block->h, pass_out_d_, out.bytes, hipMemcpyDeviceToHost, f_stream_));
        pass_bytes_flight_ = true;
        for (int o = 0; o < OBS_COUNT; ++o)
            if (n_obs[o]) { obs_counts_[o].launches.fetch_add(1, std::memory_order_relaxed); obs_counts_[o].frames.fetch_add(obs_frames[(size_t)o], std::memory_order_relaxed); }
    }
    HIP_CHECK(hipEventRecord(fb_done_[b], f_stream_));       // no host wait here: the encoder launches queue right behind
    f_unseen_by_m_ = true;
    return block ? block->h : nullptr;
}

void Engine::release_pass_block(const uint8_t *p) { for (PassBlock &b : pass_blocks_) if (b.h == p) b.busy = false; }

// a table's upload: allocated, copied under the legacy lock, freed with table_allocs_ (rs_mu_ held by the caller)
const float *Engine::upload_table(const std::vector<float> &t)
{
    HIP_CHECK(hipSetDevice(cfg_.device));
    float *d = dmalloc<float>(t.size());
    HipLegacyLock legacy;
    if (!t.empty()) HIP_CHECK(hipMemcpy(d, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
    table_allocs_.push_back(d);
    return d;
}

// the DTMF tables of this engine's model (dtmf.h), uploaded at the first DTMF pass or debug call
const float *Engine::dtmf_tables()
{
    std::lock_guard<std::mutex> g(rs_mu_);
    if (dt_tables_) return dt_tables_;
    const int wd = dtmf_window(P_.sample_rate, ft_.padded);
    if (!wd) { LOGE("DTMF on a model it refuses"); abort(); }
    std::vector<float> t((size_t)kDtmfRows * (size_t)wd);
    dtmf_make_tables(P_.sample_rate, wd, t.data());
    dt_wd_ = wd; dt_tables_ = upload_table(t);
    return dt_tables_;
}

// the tone tables of this engine's model (tone.h), uploaded at the first tone pass or debug call
const float *Engine::tone_tables()
{
    std::lock_guard<std::mutex> g(rs_mu_);
    if (tn_tables_) return tn_tables_;
    int w, k_lo, f;
    if (!tone_grid(P_.sample_rate, ft_.padded, &w, &k_lo, &f)) { LOGE("tones on a model the detector refuses"); abort(); }
    std::vector<float> t((size_t)2 * (size_t)f * (size_t)w);
    tone_make_tables(w, k_lo, f, t.data());
    tn_w_ = w; tn_f_ = f; tn_tables_ = upload_table(t);
    return tn_tables_;
}

const float *Engine::resample_table(const ResampleSpec *spec)
{
    std::lock_guard<std::mutex> g(rs_mu_);
    auto it = rs_tables_.find(spec);
    if (it != rs_tables_.end()) return it->second;
    return rs_tables_[spec] = upload_table(spec->taps);
}

// ---------------------------------------------------------------- encoder
// Every GEMM of the encoder is stated ONCE, as the argument block of its fused form over rows [r0, r0 + rows) of the work buffers
// (row r of y / ssq / xb / u / ff / p_lm / a3 / xin belongs to row r of the step: a chunk step works on rows 0 .. n - 1, the
// layer-major stages and the wavefronts on the rows of their time steps; the sessions' slots are step_d_[0 .. m - 1]).  The chains
// differ only in how they LAUNCH the blocks: one by one (run_encoder_rows, lm_stage_layer; the row-epilogue GEMMs through
// launch_rowepi, which asks the planner) or z-batched over the active layers (sw_plan, run_lm_wavefront: force_fullk as built).
// BasicNorm never runs as a kernel: EPI_RESID_SSQ leaves y and its per-32-column sums of squares, and every consumer
// of the normalised row (the next layer's gate GEMM, its residual, encoder_proj) folds the row scale in (kernels.h).

// scale of the rows that enter layer l (l == n_layers: encoder_proj): epsilon of the BasicNorm that produced them
RowScale Engine::in_scale(int l, size_t r0) const
{
    const NetDims &d = L_.dims;
    const int G = d.d_model / SSQ_COLS;
    RowScale r; r.ssq = ssq_ + r0 * G; r.groups = G; r.inv_n = 1.0f / (float)(d.d_norm ? d.d_norm : d.d_model); r.eps = l == 0 ? L_.embed_eps : L_.norm_eps[(size_t)l - 1];
    return r;
}

// The gates GEMM [norm(y) | h_prev] x Wg in its two forms.  GATES_ALL: one launch per chunk with the fused LSTM cell (chunk steps,
// feed wavefront).  Layer-major: two launches with the SAME chains -- GATES_X, the input half for a block's rows at once,
// P = (p0 + p1) * scale (waves 0,1; the recurrent half sits the launch out), and per time step GATES_H, the recurrent half + cell,
// ((P + p2) + p3) + bias.  `waves` is the form's wave mask.
GemmArgs Engine::args_gates(int l, size_t r0, int rows, int waves) const
{
    const NetDims &d = L_.dims;
    const size_t S = (size_t)cfg_.max_slots;
    const PackedLayout::Layer &o = L_.layers[(size_t)l];
    GemmArgs g; g.a0 = y_ + r0 * d.d_model; g.lda0 = d.d_model; g.K0 = d.d_model; g.lda1 = d.d_model; g.K1 = d.d_model;
    lin(g, o.wg); g.M = rows; g.N = 4 * d.hidden; g.K = 2 * d.d_model; g.kz = 1; g.wave_mask = waves;
    if (f16_tile_) { g.a0 = reinterpret_cast<const float *>(y16_ + r0 * d.d_model); lin16(g, o.wg); }      // binary16 operands
    if (waves != GATES_H) g.x_scale = in_scale(l, r0);
    if (waves == GATES_X) {           // (a1 is never read; P stays fp32 on fp16 engines too)
        g.a1 = g.a0; g.epi = EPI_XPART; g.out = p_lm_ + r0 * 4 * d.hidden; g.ldo = 4 * d.hidden;
        return g;
    }
    g.a1 = h_ + (size_t)l * S * d.d_model; g.aidx1 = step_d_; g.epi = EPI_LSTM;
    g.out = u_ + r0 * d.hidden; g.ldo = d.hidden; g.bias = w_ + o.bg; g.c_state = c_ + (size_t)l * S * d.hidden; g.slot_idx = step_d_; g.hidden = d.hidden;
    if (waves == GATES_H) { g.p_add = p_lm_ + r0 * 4 * d.hidden; g.ldp = 4 * d.hidden; }      // (a0 is never read)
    else if (cfg_.precision == 0 && gates_tile_rows(rows)) g.tile_ok = 2;      // (one problem per launch; sw_plan decides again for z-batched launches)
    if (f16_tile_) {                  // [y16 | h16(slot)], u leaves as binary16 only (its one reader is the projection)
        g.a1 = reinterpret_cast<const float *>(h16_ + (size_t)l * S * d.d_model); g.out = nullptr; g.out16 = u16_ + r0 * d.hidden;
    }
    return g;
}

// fp32 gates GEMM on the GM_TILE schedule (same chains, same bits as the hand-scheduled K-split tiles -- tests/test_gpu_gates_tile.py):
// measured 2..5 % per feed faster from ~2000 rows per launch (1024 sessions: RTF 0.0533 vs 0.055..0.058, 2048: 0.096..0.097 vs
// 0.099..0.104), slower at 256 sessions (53.5 vs 46.5 us per launch) and at one session.  APRIL_GATES_TILE: 0 never, 1 always,
// 2 (default) from GATES_TILE_MIN_ROWS rows per launch.
constexpr long GATES_TILE_MIN_ROWS = 2048;
bool Engine::gates_tile_rows(long rows) const
{
    static const int mode = env_int("APRIL_GATES_TILE", 2);
    return mode == 1 || (mode == 2 && rows >= GATES_TILE_MIN_ROWS);
}

GemmArgs Engine::args_whr(int l, size_t r0, int rows) const
{   // h' = u x Whr ; state write + residual: xb = norm(y) + h'
    const NetDims &d = L_.dims;
    const size_t S = (size_t)cfg_.max_slots;
    const PackedLayout::Layer &o = L_.layers[(size_t)l];
    GemmArgs g; g.a0 = u_ + r0 * d.hidden; g.lda0 = d.hidden; g.K0 = d.hidden; lin(g, o.whr);
    g.M = rows; g.N = d.d_model; g.K = d.hidden; g.kz = kz_hr_; g.tile_ok = tile_ok(); g.force_fullk = 1;
    g.epi = EPI_HR; g.state = h_ + (size_t)l * S * d.d_model; g.ld_state = d.d_model; g.slot_idx = step_d_; g.resid = y_ + r0 * d.d_model; g.ldr = d.d_model;
    g.r_scale = in_scale(l, r0);
    g.out = xb_ + r0 * d.d_model; g.ldo = d.d_model;
    if (f16_tile_) {
        g.a0 = reinterpret_cast<const float *>(u16_ + r0 * d.hidden); lin16(g, o.whr); g.kz = kzx_hr_;
        g.state16 = h16_ + (size_t)l * S * d.d_model; g.out16 = xb16_ + r0 * d.d_model;
    }
    return g;
}

GemmArgs Engine::args_ff1(int l, size_t r0, int rows) const
{   // FFN up + DoubleSwish
    const NetDims &d = L_.dims;
    const PackedLayout::Layer &o = L_.layers[(size_t)l];
    GemmArgs g; g.a0 = xb_ + r0 * d.d_model; g.lda0 = d.d_model; g.K0 = d.d_model; lin(g, o.wff1);
    g.M = rows; g.N = d.ffn; g.K = d.d_model; g.kz = 1; g.epi = EPI_BIAS_DSWISH; g.out = ff_ + r0 * d.ffn; g.ldo = d.ffn; g.bias = w_ + o.bff1;
    if (f16_tile_) { g.a0 = reinterpret_cast<const float *>(xb16_ + r0 * d.d_model); lin16(g, o.wff1); g.out = nullptr; g.out16 = ff16_ + r0 * d.ffn; }
    return g;
}

GemmArgs Engine::args_ff2(int l, size_t r0, int rows) const
{   // FFN down + bias + residual -> y, ssq (the last reader of the previous y was the projection)
    const NetDims &d = L_.dims;
    const PackedLayout::Layer &o = L_.layers[(size_t)l];
    GemmArgs g; g.a0 = ff_ + r0 * d.ffn; g.lda0 = d.ffn; g.K0 = d.ffn; lin(g, o.wff2);
    g.M = rows; g.N = d.d_model; g.K = d.ffn; g.kz = kz_ff2_; g.tile_ok = tile_ok(); g.force_fullk = 1;
    g.epi = EPI_RESID_SSQ; g.bias = w_ + o.bff2; g.resid = xb_ + r0 * d.d_model; g.ldr = d.d_model; g.out = y_ + r0 * d.d_model; g.ldo = d.d_model; g.ssq_out = ssq_ + r0 * (d.d_model / SSQ_COLS);
    if (f16_tile_) { g.a0 = reinterpret_cast<const float *>(ff16_ + r0 * d.ffn); lin16(g, o.wff2); g.kz = kzx_ff2_; g.out16 = y16_ + r0 * d.d_model; }
    return g;
}

GemmArgs Engine::args_encproj(size_t r0, int rows, const int *slot_idx, float *out) const
{   // encoder_proj(norm(y)) -> out[slot] (out[row] without slot_idx); fp32 A on every engine
    const NetDims &d = L_.dims;
    GemmArgs g; g.a0 = y_ + r0 * d.d_model; g.lda0 = d.d_model; g.K0 = d.d_model; lin(g, L_.w_encproj);
    g.M = rows; g.N = d.joiner; g.K = d.d_model; g.kz = kz_proj_; g.tile_ok = tile_ok();
    g.epi = EPI_SLOT_STORE; g.bias = w_ + L_.b_encproj; g.out = out; g.ldo = d.joiner; g.slot_idx = slot_idx; g.x_scale = in_scale(d.n_layers, r0);
    return g;
}

// (partial_form / row_form -- the partial-plane form of a row-epilogue GEMM and the row problem that finishes it: rowepi_forms.h)

// One row-epilogue GEMM outside the z-batched chains: its fused form when the plan (asked with `force`: take the full-K plan even
// when it yields few workgroups) keeps all of K in the workgroup, else partial planes into `ws` + the row kernel.
// cls: the launches' timing class, T_GEMM_OTHER (its row kernel: T_ROW) or T_DEC (both).
void Engine::launch_rowepi(GemmArgs f, float *ws, hipStream_t st, bool force, int cls)
{
    const int row_cls = cls == T_DEC ? T_DEC : T_ROW;
    f.force_fullk = force ? 1 : 0;
    const GemmPlan p = gemm_plan(f);
    if (p.fused) { timed_begin(cls); launch_gemm(f, st); timed_end(cls); return; }
    timed_begin(cls); launch_gemm(partial_form(f, ws, ws_mstride_), st); timed_end(cls);
    timed_begin(row_cls); launch_row(row_form(f, ws, ws_mstride_, p.planes), st); timed_end(row_cls);
}

// conv front end + embed linear of rows [r0, r0 + rows) -> y, ssq (and y16: layer 0 of an fp16 tile engine reads binary16 rows).
// row_slots: the slot of every row, from row 0; ring tails: index array [1]; split-K planes of the embed GEMM, if any, go to `ws`
void Engine::encoder_front(size_t r0, int rows, const int *row_slots, const float *x_direct, hipStream_t st, float *ws)
{
    const NetDims &d = L_.dims;
    ConvEmbedArgs ca;
    ca.ring = ring_; ca.ring_frames = ring_frames_; ca.mel = d.mel; ca.seg = d.seg;
    ca.slot_idx = row_slots + r0; ca.ring_tail = step_d_ + cfg_.max_batch + r0; ca.x_direct = x_direct;
    for (int i = 0; i < 3; ++i) { ca.w[i] = w_ + L_.conv_w[i]; ca.b[i] = w_ + L_.conv_b[i]; ca.ch[i] = d.conv_ch[i]; ca.stride[i] = d.conv_stride[i]; }
    ca.ch1_per_group = conv_ch1_per_group(d.conv_ch[1]);
    ca.out = a3_ + r0 * d.f_out * L_.k3; ca.ldo = L_.k3; ca.M = rows;
    if (conv_wt_) { ca.w0t = conv_wt_; ca.w1t = conv_wt_ + (size_t)9 * d.conv_ch[0]; }
    timed_begin(T_CONV); launch_conv_embed(ca, st); timed_end(T_CONV);
    {   // third conv: [rows * f_out, k3] x [k3, c2] + bias, DoubleSwish -> xin[rows][f_out * c2]
        GemmArgs g; g.a0 = ca.out; g.lda0 = L_.k3; g.K0 = L_.k3; g.wp = w_ + L_.conv_w[2];
        g.M = rows * d.f_out; g.N = d.conv_ch[2]; g.K = L_.k3; g.kz = 1; g.epi = EPI_BIAS_DSWISH; g.out = xin_ + r0 * d.embed_in; g.ldo = d.conv_ch[2]; g.bias = w_ + L_.conv_b[2];
        timed_begin(T_CONV); launch_gemm(g, st); timed_end(T_CONV);
    }
    {   // embed linear + bias -> y, ssq (BasicNorm deferred); fp32 A on every engine
        GemmArgs g; g.a0 = xin_ + r0 * d.embed_in; g.lda0 = d.embed_in; g.K0 = d.embed_in; lin(g, L_.w_embed);
        g.M = rows; g.N = d.d_model; g.K = d.embed_in; g.kz = kz_embed_; g.tile_ok = tile_ok();
        g.epi = EPI_RESID_SSQ; g.bias = w_ + L_.b_embed; g.ldr = d.d_model; g.out = y_ + r0 * d.d_model; g.ldo = d.d_model; g.ssq_out = ssq_ + r0 * (d.d_model / SSQ_COLS);
        launch_rowepi(g, ws + r0 * d.d_model, st);
    }
    if (f16_tile_) launch_cvt_f16(y_ + r0 * d.d_model, y16_ + r0 * d.d_model, (size_t)rows * d.d_model, st);
}

// One chunk for n sessions on rows 0 .. n - 1 (slots step_d_[0 .. n - 1]).  Launch count per chunk at batch sizes where the
// full-K schedule applies: 2 (conv) + 1 (embed) + 4 per layer + 1.
void Engine::run_encoder_rows(int n, const float *x_direct)
{
    const NetDims &d = L_.dims;
    encoder_front(0, n, step_d_, x_direct, stream_, ws_);
    for (int l = 0; l < d.n_layers; ++l) {
        timed_begin(T_GATES); launch_gemm(args_gates(l, 0, n, GATES_ALL), stream_); timed_end(T_GATES);
        launch_rowepi(args_whr(l, 0, n), ws_, stream_);
        timed_begin(T_GEMM_OTHER); launch_gemm(args_ff1(l, 0, n), stream_); timed_end(T_GEMM_OTHER);
        launch_rowepi(args_ff2(l, 0, n), ws_, stream_);
    }
    launch_rowepi(args_encproj(0, n, step_d_, eout_), ws_, stream_);
}

// ---------------------------------------------------------------- decoder / joiner rounds
DecEmbedParams Engine::dec_params() const
{
    const NetDims &d = L_.dims;
    DecEmbedParams p; p.emb = w_ + L_.emb; p.conv_w = w_ + L_.dec_conv; p.conv_b = L_.has_dec_conv_b ? w_ + L_.dec_conv_b : nullptr;
    p.d = d.d_model; p.groups = d.dec_groups; p.context = d.context; p.vocab = d.vocab;
    return p;
}

// dout[slot] = de x Wp + b for rows with row_mask != 0 (all rows when null), on the search's stream and workspace
void Engine::run_decproj(int n, const int *d_slots, const int *row_mask, const int *run_flag, int run_gen, float *out)
{
    const NetDims &d = L_.dims;
    GemmArgs g; g.a0 = de_; g.lda0 = d.d_model; g.K0 = d.d_model; lin(g, L_.w_decproj);
    g.M = n; g.N = d.joiner; g.K = d.d_model; g.kz = kz_proj_; g.tile_ok = tile_ok(); g.run_flag = run_flag; g.run_gen = run_gen;
    g.epi = EPI_SLOT_STORE; g.bias = w_ + L_.b_decproj; g.out = out ? out : dout_; g.ldo = d.joiner; g.slot_idx = d_slots; g.row_mask = row_mask;
    launch_rowepi(g, ws_g_, search_stream_, false, T_DEC);
}

// The reference's loop "joiner -> process_logits, up to three times, early-emit 1,0,0" (src/april_session.c:449-454)
// for all rows of the step at once, decisions included: rows that resolved to blank are masked out of the later rounds.
void Engine::run_greedy_rounds(int n, bool dump_logits, int chunk, const float *eout_rows)
{
    const int MB = cfg_.max_batch;
    GreedyIo io;
    io.gen = chunk + 1; io.now = step_d_ + 2 * MB + (size_t)chunk * n; io.eout = eout_rows; io.rec_off = rec_off_d_; io.rec_slot0 = chunk * 3;
    io.dump = dump_logits ? logits_ + (size_t)chunk * 3 * n * L_.dims.vocab : nullptr;
    run_greedy_rounds(n, io);
}

void Engine::run_greedy_rounds(int n, const GreedyIo &io)
{
    const NetDims &d = L_.dims;
    const int gen = io.gen;
    const int *d_slots = step_d_;
    for (int round = 0; round < 3; ++round) {
        int planes;
        {   // logits = tanh(eout + dout) x Wout (+ bias in the decision kernel)
            GemmArgs g; g.a0b = dout_; g.lda0 = d.joiner; g.K0 = d.joiner; g.a_op = AOP_TANH_ADD;
            if (dec_table_) { g.a0b = dec_table_; g.ctx_state = gstate_; g.ctx_vocab = d.vocab; }     // dout = the table row of the slot's context
            if (io.eout) { g.a0 = io.eout; g.aidx0 = io.eout_rows; g.same_idx_b = 0; g.aidx0b = d_slots; }     // layer-major: this chunk's rows of the batched encoder output
            else { g.a0 = eout_; g.aidx0 = d_slots; }
            lin(g, L_.w_out); g.M = n; g.N = L_.vocab_pad; g.K = d.joiner; g.kz = kz_out_; g.epi = EPI_PARTIAL; g.out = ws_g_; g.m_stride = ws_mstride_;
            if (round > 0) { g.run_flag = flags_d_ + round; g.run_gen = gen; }
            planes = gemm_plan(g).planes;
            timed_begin(T_DEC); launch_gemm(g, search_stream_); timed_end(T_DEC);
        }
        DecideArgs a;
        a.ws = ws_g_; a.parts = planes; a.m_stride = ws_mstride_; a.N = L_.vocab_pad; a.M = n; a.n_valid = d.vocab;
        a.bias = w_ + L_.b_out; a.blank = P_.blank_id; a.early_emit = round == 0 ? 1.0f : 0.0f;
        a.slot_idx = d_slots; a.now_ms = io.now; a.active = active_d_; a.dirty = dirty_d_; a.tok_class = cls_; a.state = gstate_;
        a.rec_ring = rec_d_; a.rec_off = io.rec_off; a.round = round; a.gen = gen; a.rec_slot = io.rec_slot0 + round;
        a.logits_dump = io.dump ? io.dump + (size_t)round * n * d.vocab : nullptr;
        a.dec = dec_params(); a.de_out = dec_table_ ? nullptr : de_; a.ld_de = d.d_model;
        a.run_flags = flags_d_; a.rerun_flags = flags_d_ + 4;
        a.conf_k = conf_k_.d; a.conf_ring = conf_d_;          // (null until a session of this engine asks for confidences)
        a.bias_set = bias_set_.d; a.bias_state = bias_state_d_; a.bias_desc = bias_desc_.d;      // (null until a session of this engine has a bias set)
        a.opt = opt_.d;                                        // (null until a session of this engine has search options)
        if (lm_slot_.d) { a.lm_slot = lm_slot_.d; a.lm_state = lm_state_d_; a.lm_desc = lm_desc_.d; lm_launches_.fetch_add(1, std::memory_order_relaxed); }      // (null until a session of this engine has a language model)
        timed_begin(T_DEC); launch_decide(a, search_stream_); timed_end(T_DEC);
        if (!dec_table_) run_decproj(n, d_slots, dirty_d_, flags_d_ + 4 + round, gen);
    }
}

// the index fetch of a step: T == 0: a chunk step, three arrays of m (slots, ring tails, session times); else the layer-major
// arrays (below) of T chunks of m sessions
AdvanceArgs Engine::advance_args(int m, int T) const
{
    AdvanceArgs a;
    a.host_ring = ring_h_; a.host_step_off = step_off_h_; a.host_rec_off = rec_off_h_; a.counter = counter_d_; a.index_mask = 2 * step_cap_ - 1;
    a.dst = step_d_; a.dst_stride = cfg_.max_batch; a.n_arrays = T ? 4 : 3; a.len[0] = m;
    for (int i = 1; i < a.n_arrays; ++i) a.len[i] = T ? m * T : m;
    a.rec_off = rec_off_d_; a.flags = flags_d_; a.n_flags = 8;
    return a;
}

void Engine::run_chain(int m, bool dump_logits)
{
    launch_advance(advance_args(m, 0), stream_);
    run_encoder_rows(m, nullptr);
    run_greedy_rounds(m, dump_logits);
}

// ---------------------------------------------------------------- layer-major step
// Index arrays on the device (stride max_batch): [0] slots (m), [1] ring tails (T x m), [2] session times (T x m),
// [3] slot of every row (T x m).  Row r = t * m + i.  The work is cut into STAGES over a block of time steps [t0, t1):
//   front(block)      conv front end + embed linear (encoder_front)   -> y, ssq rows of the block
//   layer(l, block)   input half of the gates for the block's rows at once; per time step recurrent half + cell and the
//                     projection; feed-forward over the block's rows   -> y, ssq rows of the block
//   proj(block)       encoder_proj                                   -> eout_lm rows of the block
// layer(l, b) needs layer(l - 1, b) (its input rows) and layer(l, b - 1) (the recurrent state): stages of different layers
// on different blocks are independent: their launches are z-batched into one (see run_lm_wavefront).  Work buffers are row-partitioned
// (the split-K planes too: a stage's planes lie at its first row's d_model-wide slice of the workspace), so concurrent stages never
// share a byte.
void Engine::lm_stage_layer(int l, int m, int t0, int t1, hipStream_t st)
{
    const NetDims &d = L_.dims;
    const size_t b0 = (size_t)t0 * m;
    const int brows = (t1 - t0) * m;
    timed_begin(T_GATES); launch_gemm(args_gates(l, b0, brows, GATES_X), st); timed_end(T_GATES);
    for (int t = t0; t < t1; ++t) {
        const size_t r0 = (size_t)t * m;
        timed_begin(T_GATES); launch_gemm(args_gates(l, r0, m, GATES_H), st); timed_end(T_GATES);
        // (sequential step: on the K-split kernels one launch however few workgroups; the fp16 tile kernels by the planner's choice)
        launch_rowepi(args_whr(l, r0, m), ws_ + r0 * d.d_model, st, !f16_tile_);
    }
    timed_begin(T_GEMM_OTHER); launch_gemm(args_ff1(l, b0, brows), st); timed_end(T_GEMM_OTHER);
    launch_rowepi(args_ff2(l, b0, brows), ws_ + b0 * d.d_model, st);
}

void Engine::lm_stage_proj(int m, int t0, int t1, hipStream_t st, float *ws)
{
    const NetDims &d = L_.dims;
    const size_t b0 = (size_t)t0 * m;
    // (joiner width == a d_model-wide slice or less: see the constructor's workspace size)
    launch_rowepi(args_encproj(b0, (t1 - t0) * m, nullptr, eout_lm_ + b0 * d.joiner), ws + b0 * d.d_model, st, true);
}

// Time steps per block of the long-feed wavefront (run_lm_wavefront).  A macro step costs its block's recurrent launches (2 per
// time step, whatever the number of active layers) plus ~80 us of block stages (input halves, feed-forward, front end: weight
// streams that do not depend on the block length), and the wavefront runs NB + L + 1 macro steps, L + 1 of them fill / drain:
// (T / blk + L + 1) (c_step blk + c_block) is smallest near blk = sqrt(T c_block / ((L + 1) c_step)) ~ 0.75 sqrt(T) at aprilv0
// size.  Measured, 60 s in one call (T = 1498): blk 10 / 16 / 20 / 24 / 32 -> 65.5 / 61.6 / 61.2 / 60.6 / 60.2 ms.
// Results do not depend on the block length (same chains in the same order).
static int lm_block_steps(int T)
{
    const int b = (int)(0.75 * std::sqrt((double)std::max(1, T)) + 0.5);
    return std::max(6, std::min(32, b));
}
// (feeds up to this many chunks run as one layer-major chain, captured as a graph: too few blocks for a wavefront to fill)
constexpr int LM_WAVEFRONT_MIN_CHUNKS = 10;

static bool lm_wavefront_on()
{
    static const bool on = env_int("APRIL_LM_WAVEFRONT", 1) != 0;
    return on;
}

void Engine::run_lm_chain(int m, int T, bool dump_logits)
{
    const NetDims &d = L_.dims;
    const int MB = cfg_.max_batch;
    const int L = d.n_layers;
    launch_advance(advance_args(m, T), stream_);
    encoder_front(0, m * T, step_d_ + 3 * MB, nullptr, stream_, ws_);
    for (int l = 0; l < L; ++l) lm_stage_layer(l, m, 0, T, stream_);
    lm_stage_proj(m, 0, T, stream_, ws_);
    // the search stays sequential in time (the decoder input of chunk t + 1 depends on the tokens of chunk t)
    for (int t = 0; t < T; ++t) run_greedy_rounds(m, dump_logits, t, eout_lm_ + (size_t)t * m * d.joiner);
}

// Wavefront form of the layer-major step (long feeds: T > block).  Time is cut into blocks of `blk` steps; at macro step W
// layer l works on block W - 1 - l, the front end on block W, encoder_proj on block W - L - 1 -- all of them independent of
// one another.  The SAME launch of different layers is therefore ONE launch (gemm_f32_zkernel: blockIdx.z picks the layer's
// argument block): per macro step one launch for the input halves of the gates, 2 per time step of the block for the
// recurrence, one each for the feed-forward GEMMs -- (2 blk + 3) launches for L layer stages instead of L (2 blk + 3), on ONE
// stream, no cross-stream events.  At one session every recurrent kernel is a latency-bound launch of a few microseconds, and
// twelve of them in one launch cost about the same as one.  The search (sequential in time) follows on the engine's stream,
// one block behind, as ONE captured graph per block whose arguments do not depend on the block (launch_block_setup).
// Arithmetic: the kernels and their arguments are those of lm_stage_layer; only the grouping into launches differs.
void Engine::run_lm_wavefront(int m, int T, bool dump_logits)
{
    const NetDims &d = L_.dims;
    const int MB = cfg_.max_batch;
    const int L = d.n_layers;
    const int blk = lm_block_steps(T);
    const int NB = (T + blk - 1) / blk;
    launch_advance(advance_args(m, T), stream_);
    hipStream_t cs = lm_stream_;
    HIP_CHECK(hipEventRecord(lm_events_[0], stream_));                 // the index block is on the device
    HIP_CHECK(hipStreamWaitEvent(cs, lm_events_[0], 0));

    // argument blocks of this step: (NB + L + 1) macro steps x at most (2 blk + 6) launches x L layers, in one of three
    // regions that are reused round robin once the step that used them has run (the host runs ahead of the GPU by whole steps)
    const size_t need = (size_t)(NB + L + 1) * (size_t)(2 * blk + 6) * (size_t)L;
    if (need > zargs_region_) {
        HIP_CHECK(hipStreamSynchronize(cs));
        HipLegacyLock regrow_guard;                   // (see fbank())
        if (zargs_h_) { (void)hipHostFree(zargs_h_); (void)hipFree(zargs_d_); }
        zargs_region_ = need + need / 4;
        zargs_h_ = hmalloc<GemmArgs>(3 * zargs_region_); zargs_d_ = dmalloc<GemmArgs>(3 * zargs_region_);
        for (int i = 0; i < 3; ++i) zargs_busy_[i] = false;
    }
    const int zslot = zargs_next_;
    zargs_next_ = (zargs_next_ + 1) % 3;
    if (zargs_busy_[zslot]) HIP_CHECK(hipEventSynchronize(zargs_done_[zslot]));
    zargs_pos_ = (size_t)zslot * zargs_region_;

    static const bool timing = env_str("APRIL_LM_TIMING") != nullptr;        // measurement: host time of the enqueue by part
    double tacc[6] = {0, 0, 0, 0, 0, 0};
    auto now = [&]() { return timing ? std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count() : 0.0; };
    struct Batch { size_t off; int n; };
    std::vector<Batch> plan;                               // the z-batched launches of all macro steps, in order
    std::vector<size_t> plan_end((size_t)(NB + L + 1), 0); // macro step W owns plan[plan_end[W - 1] .. plan_end[W])
    std::vector<GemmArgs> items;
    struct Act { int l, t0, t1; };
    std::vector<Act> act;
    double tq = now();
    auto lap = [&](int i) { if (timing) { const double t = now(); tacc[i] += t - tq; tq = t; } };
    // The argument blocks of the WHOLE step first, then ONE host-to-device copy: a copy between the kernels of every macro step
    // stalls the stream each time (measured: 13 us per macro step, 2.5 ms per minute of audio); the blocks depend on (m, T) and
    // buffer addresses only.
    const size_t first = zargs_pos_;
    for (int W = 0; W <= NB + L; ++W) {
        act.clear();
        for (int l = 0; l < L; ++l) { const int b = W - 1 - l; if (b >= 0 && b < NB) act.push_back({l, b * blk, std::min(T, (b + 1) * blk)}); }
        auto flush = [&]() {
            if (items.empty()) return;
            stage_gemm_z(items.data(), (int)items.size(), zargs_h_ + zargs_pos_);
            plan.push_back({zargs_pos_, (int)items.size()});
            zargs_pos_ += items.size(); items.clear();
        };
        // the block stages come in at most two lengths (full blocks, the tail): one launch per length
        auto by_len = [&](auto make) {
            for (int pass = 0; pass < 2; ++pass) {
                for (const Act &x : act) if (((x.t1 - x.t0) == blk) == (pass == 0)) items.push_back(make(x));
                flush();
            }
        };
        by_len([&](const Act &x) { return args_gates(x.l, (size_t)x.t0 * m, (x.t1 - x.t0) * m, GATES_X); });
        for (int i = 0; i < blk; ++i) {
            for (const Act &x : act) if (x.t0 + i < x.t1) items.push_back(args_gates(x.l, (size_t)(x.t0 + i) * m, m, GATES_H));
            flush();
            for (const Act &x : act) if (x.t0 + i < x.t1) items.push_back(args_whr(x.l, (size_t)(x.t0 + i) * m, m));
            flush();
        }
        by_len([&](const Act &x) { return args_ff1(x.l, (size_t)x.t0 * m, (x.t1 - x.t0) * m); });
        by_len([&](const Act &x) { return args_ff2(x.l, (size_t)x.t0 * m, (x.t1 - x.t0) * m); });
        plan_end[(size_t)W] = plan.size();
    }
    lap(0);
    if (zargs_pos_ > first)
        HIP_CHECK(hipMemcpyAsync(zargs_d_ + first, zargs_h_ + first, (zargs_pos_ - first) * sizeof(GemmArgs), hipMemcpyHostToDevice, cs));
    lap(1);
    for (int W = 0; W <= NB + L; ++W) {
        if (W < NB) encoder_front((size_t)W * blk * m, (std::min(T, (W + 1) * blk) - W * blk) * m, step_d_ + 3 * MB, nullptr, cs, ws_);
        lap(2);
        for (size_t k = W ? plan_end[(size_t)W - 1] : 0; k < plan_end[(size_t)W]; ++k) launch_gemm_z(zargs_h_ + plan[k].off, plan[k].n, zargs_d_ + plan[k].off, cs);
        lap(3);
        const int bp = W - L - 1;
        if (bp >= 0) {
            const int t0 = bp * blk, t1 = std::min(T, t0 + blk), len = t1 - t0;
            lm_stage_proj(m, t0, t1, cs, ws_);
            hipEvent_t e = lm_events_[1 + (size_t)(bp % (int)(lm_events_.size() - 1))];
            HIP_CHECK(hipEventRecord(e, cs));
            HIP_CHECK(hipStreamWaitEvent(stream_, e, 0));
            // the block's search: bookkeeping at fixed places, then the block-independent launch chain
            BlockSetupArgs bs;
            bs.now_src = step_d_ + 2 * MB + (size_t)t0 * m; bs.now_dst = lm_now_d_; bs.rows_dst = lm_rows_d_; bs.row0 = t0 * m; bs.count = len * m;
            bs.rec_off_step = rec_off_d_; bs.rec_off_block = lm_rec_off_d_; bs.rec_add = t0 * 3 * m; bs.flags = flags_d_; bs.n_flags = 8;
            launch_block_setup(bs, stream_);
            lap(4);
            auto search = [&]() {
                for (int i = 0; i < len; ++i) {
                    GreedyIo io;
                    io.gen = i + 1; io.now = lm_now_d_ + (size_t)i * m; io.eout = eout_lm_; io.eout_rows = lm_rows_d_ + (size_t)i * m;
                    io.rec_off = lm_rec_off_d_; io.rec_slot0 = i * 3;
                    io.dump = dump_logits ? logits_ + (size_t)(t0 + i) * 3 * m * d.vocab : nullptr;
                    run_greedy_rounds(m, io);
                }
            };
            if (!use_graphs_ || dump_logits) { search(); continue; }
            const GraphCache::Key key = graph_key(m, len);       // (round flags and encoder outputs are per flight parity)
            if (!lm_search_graphs_.find(key) && lm_search_graphs_.full()) { HIP_CHECK(hipStreamSynchronize(stream_)); /* execs launched earlier in this flight may still run */ lm_search_graphs_.clear(); }
            HIP_CHECK(hipGraphLaunch(cached_graph(lm_search_graphs_, key, stream_, search), stream_));
            lap(5);
        }
    }
    HIP_CHECK(hipEventRecord(zargs_done_[zslot], cs));
    zargs_busy_[zslot] = true;
    if (timing) fprintf(stderr, "lm wavefront %d x %d: host us: args %.0f, arg copy %.0f, front end %.0f, layer launches %.0f, proj + events + setup %.0f, search graph %.0f\n",
                        m, T, tacc[0], tacc[1], tacc[2], tacc[3], tacc[4], tacc[5]);
}

// ---------------------------------------------------------------- chunk steps of one feed as a wavefront
// A 100 ms feed carries 2..3 chunks per session.  Chunk t + 1 of layer l does not depend on chunk t of layer l + 1, so the T
// chunk steps of a feed run as a wavefront over the layers: at macro step W layer l works on chunk W - 1 - l, and the same
// launch of the (up to T) active layers is ONE z-batched launch.  Same kernels and arguments as T chunk steps in a row
// (run_encoder_rows), on the rows of chunk t instead of rows 0..m-1: bit-identical.  What it buys: 4 (L + T - 1) layer
// launches per feed instead of 4 L T, and -- the reason it pays at 256 sessions -- a launch holds T x the workgroups, so the
// planner picks larger tiles for the N = d_model GEMMs (32x32 instead of 16x32 at 256 rows: 1.5 x fewer operand bytes per
// flop, the bound of those kernels) and co-resident workgroups overlap each other's prologue / epilogue.
// The argument blocks depend on (m, T) only: built once per shape, kept in device memory, and the whole chain is one graph.
static bool lm_gates_split_on()
{
    static const bool on = env_int("APRIL_GATES_SPLIT", 1) != 0;
    return on;
}

Engine::SwPlan &Engine::sw_plan(int m, int T)
{
    const GraphCache::Key key = sw_key(m, T);         // (the argument blocks point into the parity's buffers)
    auto it = sw_plans_.find(key);
    if (it != sw_plans_.end()) return it->second;
    if (sw_plans_.size() >= sw_plan_cap_) {
        sync();
        HipLegacyLock evict_guard;                    // (see fbank())
        collect_gates_clock(); free_sw_plans();       // the stamp slots of the clocked plans go with them: their sums first, ...
        if (gclk_slots_) { HIP_CHECK(hipMemsetAsync(gclk_slots_, 0, (size_t)GCLK_SLOTS * STAMP_WORDS * 8, stream_)); HIP_CHECK(hipStreamSynchronize(stream_)); }
        gclk_used_ = 0;                               // ... then every slot is free again
    }
    SwPlan &p = sw_plans_[key];
    build_sw_chain(p, p.one, m, T, false);
    // (clocked runs never take the split flavour: run_feed_wavefront)
    if (ramp_mode_ != 0 && !gclk_) build_sw_chain(p, p.split, m, T, true);
    if (ramp_mode_ == 1 && !gclk_ && L_.dims.n_layers > 2 * RAMP_R) build_sw_chain(p, p.headless, m, T, true, true);      // (L <= 2 R: nobody hosts, ramp_window)
    return p;
}

// ---------------------------------------------------------------- ramp merge
// The first and the last macro steps of a feed's wavefront hold one or two problems per launch, and a launch costs ~27 us whatever
// it holds.  Under the pipelined ingest the next feed's front end is through long before this feed's layers reach their tail, so
// the tail [2, 1] of feed k and the head [1, 2] of feed k + 1 run as [3, 3]: the split-flavour plan of (m, T, parity p) carries, in
// its last RAMP_R macro steps, GUEST argument blocks for the first RAMP_R macro steps of a feed of m sessions of the other parity
// (their rows t * m in that parity's buffers: they depend on m only).  Guest blocks run only when the word the latch kernel wrote
// for them holds 1.  The decision is the device's (kernels_misc.hip, ramp_latch_kernel); the scheduler knows nothing of it.
// APRIL_RAMP_MERGE=1: the latch reports the decision to the host, which enqueues the hosted feed's layer graph only then, and without the
// head steps ("deferred enqueue", below).  =3 / =2, the guarded forms: the next feed's graph is enqueued at once, and the own blocks of
// every split plan's first RAMP_R macro steps run only while head_live[p] holds 1.
std::vector<RampStep> ramp_window(int L, int T, int R, int max_problems)
{
    std::vector<RampStep> w;
    if (L <= 2 * R || T < 1 || R < 1) return w;
    for (int j = 1; j <= R; ++j) {
        RampStep s; s.macro = L + T - 1 - R + j;
        for (int l = 0; l < L; ++l) { const int t = s.macro - 1 - l; if (t >= 0 && t < T) ++s.own; }
        for (int t = 0; t < j; ++t) s.guests.push_back(std::make_pair(j - 1 - t, t));
        if (s.own + (int)s.guests.size() > max_problems) return std::vector<RampStep>();
        w.push_back(s);
    }
    return w;
}

void Engine::ramp_counts(uint64_t *hosted, uint64_t *eligible)
{
    unsigned h = 0;
    {
        HipLegacyLock legacy;                         // (a legacy-stream copy: not while an engine captures a graph, see engine.h)
        if (hipSetDevice(cfg_.device) == hipSuccess) HIP_CHECK(hipMemcpy(&h, &ramp_d_->hosted, sizeof h, hipMemcpyDeviceToHost));
    }
    *hosted = h; *eligible = ramp_eligible_.load(std::memory_order_relaxed);
}

// ramp: the split flavour (latch, guest window).  Its head steps sit behind head_live in the guarded forms only (APRIL_RAMP_MERGE=3 / 2); with the deferred enqueue
// the chain with the head is launched only where the head runs.  headless: the same chain from macro step RAMP_R + 1 on -- same blocks, forms and staging.
void Engine::build_sw_chain(SwPlan &p, SwPlan::Chain &c, int m, int T, bool ramp, bool headless)
{
    const bool guard = ramp && ramp_mode_ != 1;
    const NetDims &d = L_.dims;
    const int L = d.n_layers;
    const int par = flight_parity_;
    // Does a launch of n problems of this kind need a row finisher, and over how many planes?  (Projection and FFN down on the GM_TILE
    // schedule, see below.)  The chain asks without force: GM_TILE's K cut is a matter of occupancy; every other plan is launched
    // fused, forced (force_fullk as args_whr / args_ff2 build it).
    auto needs_rows = [&](int kind, int n) {
        if (kind != 1 && kind != 3) return 0;
        GemmArgs g = kind == 1 ? args_whr(0, 0, m) : args_ff2(0, 0, m);
        g.force_fullk = 0; g.zcount = n;
        const GemmPlan p = gemm_plan(g);
        return p.mode == GM_TILE && !p.fused ? p.planes : 0;
    };
    // hosting: own + guest problems fit the three-problem forms in both window steps and no launch of the window needs a row finisher
    std::vector<RampStep> window;
    if (ramp && m <= RAMP_MAX_M && T <= RAMP_MAX_T) {
        window = ramp_window(L, T, RAMP_R);
        for (const RampStep &s : window) if (needs_rows(1, s.own + (int)s.guests.size()) || needs_rows(3, s.own + (int)s.guests.size())) { window.clear(); break; }
    }
    if (ramp) p.hosts = !window.empty();
    std::vector<GemmArgs> items;
    std::vector<RowArgs> rows;
    for (int W = headless ? RAMP_R + 1 : 0; W <= T + L; ++W) {
        const RampStep *host = nullptr; int wj = 0;
        for (size_t j = 0; j < window.size(); ++j) if (window[j].macro == W) { host = &window[j]; wj = (int)j; }
        if (host && wj == 0) { SwPlan::Batch b; b.off = c.host.size(); b.n = 0; b.macro = W; b.kind = 4; b.roff = c.rhost.size(); b.rn = 0; c.batches.push_back(b); }      // the latch
        for (int kind = 0; kind < 4; ++kind) {
            items.clear(); rows.clear();
            int n_act = 0;
            for (int l = 0; l < L; ++l) { const int t = W - 1 - l; if (t >= 0 && t < T) ++n_act; }
            if (n_act == 0) continue;
            if (host) n_act += (int)host->guests.size();      // (planned and staged for own + guest problems)
            // The N = d_model GEMMs (projection, FFN down) on the GM_TILE schedule: when the n_act problems of this launch give the
            // chip too few 64 x 64 tiles, K is cut across workgroups and ONE z-batched row launch finishes the slab tree with the
            // epilogue (state write + residual / bias + residual + sums of squares) -- the same arithmetic as the fused form.
            const int planes = needs_rows(kind, n_act);
            const bool split = planes > 0;
            auto problem = [&](int l, int t, const int *run_flag) {
                const size_t r0 = (size_t)t * m;
                GemmArgs g = kind == 0 ? args_gates(l, r0, m, GATES_ALL) : kind == 1 ? args_whr(l, r0, m) : kind == 2 ? args_ff1(l, r0, m) : args_ff2(l, r0, m);
                if (kind == 0 && cfg_.precision == 0) g.tile_ok = gates_tile_rows((long)m * n_act) ? 2 : 0;
                if (run_flag) { g.run_flag = run_flag; g.run_gen = 1; }
                if (split) {
                    float *ws = ws_ + r0 * d.d_model;
                    rows.push_back(row_form(g, ws, ws_mstride_, planes));
                    g = partial_form(g, ws, ws_mstride_);
                } else if (f16_tile_) g.force_fullk = 0;      // (launched as asked: GM_TILE always takes an fp16 tile GEMM)
                items.push_back(g);
            };
            for (int l = 0; l < L; ++l) {
                const int t = W - 1 - l;
                if (t < 0 || t >= T) continue;
                problem(l, t, guard && W <= RAMP_R ? &ramp_d_->head_live[par] : nullptr);
            }
            if (host) {
                select_parity(1 - par);
                for (const auto &lt : host->guests) problem(lt.first, lt.second, &ramp_d_->guest_live[par][wj][lt.second]);
                select_parity(par);
            }
            // The gates launch of four and more problems (merged flights: two feeds stepped as one wavefront of up to seven chunk steps) goes
            // out as launches of two or three: the hand-scheduled 64 x 64 kernel holds 512 workgroups at a time, two problems are exactly one
            // round and three run on walking workgroups, while four to six in one grid measured 82.5 / 110 / 125 us against 76.8 / 97.3 / 117.8
            // for the pieces (rocprofv3 by grid size, round 6) -- and every launch of a kernel name then holds one problem count, which is
            // what makes a per-kernel trace comparable with the gates clock.  (fp32, below the GM_TILE row count only.)
            std::vector<int> groups;
            {
                int left = (int)items.size();
                const bool cut = kind == 0 && cfg_.precision == 0 && left >= 4 && !gates_tile_rows((long)m * n_act) && lm_gates_split_on();
                while (cut && left > 0) { const int take = (left == 4 || left == 2) ? 2 : (left >= 3 ? 3 : left); groups.push_back(take); left -= take; }
                if (groups.empty()) groups.push_back((int)items.size());
            }
            size_t first = 0;
            for (size_t gi = 0; gi < groups.size(); ++gi) {
                const int gn = groups[gi];
                if (kind == 0 && !ramp && gclk_ && gclk_slots_ && gclk_used_ < GCLK_SLOTS) {      // one slot per gates LAUNCH: all its problems point at it
                    p.stamp_slots.push_back(std::make_pair(gclk_used_, (long)m * gn)); p.stamp_n.push_back(gn);
                    for (int i = 0; i < gn; ++i) items[first + (size_t)i].stamp = gclk_slots_ + (size_t)gclk_used_ * STAMP_WORDS;
                    ++gclk_used_;
                } else if (kind == 0 && !ramp && gclk_ && gclk_slots_ && !gclk_warned_) {
                    gclk_warned_ = true; LOGW("engine: the gates clock is out of stamp slots (%d): the gates launches of further plans are not timed", GCLK_SLOTS);
                }
                SwPlan::Batch b; b.off = c.host.size(); b.n = gn; b.macro = W; b.kind = kind; b.roff = c.rhost.size(); b.rn = gi == 0 ? (int)rows.size() : 0;
                c.host.resize(c.host.size() + (size_t)gn);
                stage_gemm_z(items.data() + first, gn, c.host.data() + b.off);
                if (gi == 0) c.rhost.insert(c.rhost.end(), rows.begin(), rows.end());
                c.batches.push_back(b);
                first += (size_t)gn;
            }
        }
    }
    m_touched();
    c.dev = dmalloc<GemmArgs>(c.host.size());
    // (stream-ordered on the engine's own stream: a blocking hipMemcpy goes through the legacy stream, which HIP refuses while
    // ANOTHER engine's stepping thread is capturing a graph -- two engines on one device, several models in one process)
    HIP_CHECK(hipMemcpyAsync(c.dev, c.host.data(), c.host.size() * sizeof(GemmArgs), hipMemcpyHostToDevice, stream_));
    if (!c.rhost.empty()) {
        c.rdev = dmalloc<RowArgs>(c.rhost.size());
        HIP_CHECK(hipMemcpyAsync(c.rdev, c.rhost.data(), c.rhost.size() * sizeof(RowArgs), hipMemcpyHostToDevice, stream_));
    }
}

void Engine::free_sw_plans()
{
    if (!sw_plans_.empty()) LOGI("engine: feed wavefront plans emptied (%zu plans)", sw_plans_.size());
    for (auto &p : sw_plans_) for (SwPlan::Chain *c : {&p.second.one, &p.second.split, &p.second.headless}) { if (c->dev) (void)hipFree(c->dev); if (c->rdev) (void)hipFree(c->rdev); }
    sw_graphs_.clear(); sw_plans_.clear();
}

// part 0: index fetch + front end (stream fe), 1: the layer wavefront (stream ly), 2: encoder_proj + the searches (stream sr), 3: the headless
// layer wavefront (stream ly); parts < 0: the first three in order on one stream
void Engine::run_sw_chain(int m, int T, bool dump_logits, const SwPlan &p, int part, hipStream_t st)
{
    const NetDims &d = L_.dims;
    const int MB = cfg_.max_batch;
    if (part < 0 || part == 0) {
        launch_advance(advance_args(m, T), st);
        // Front end and encoder_proj do not take part in the wavefront: one launch chain each over all T x m rows (as in the
        // layer-major step), before the first and after the last macro step; the searches follow in time order.
        encoder_front(0, m * T, step_d_ + 3 * MB, nullptr, st, part == 0 ? ws_fe_ : ws_);
    }
    if (part < 0 || part == 1 || part == 3) {
        static const int cls_of[4] = {T_GATES, T_GEMM_OTHER, T_GEMM_OTHER, T_GEMM_OTHER};
        const SwPlan::Chain &c = part == 3 ? p.headless : p.layers(part == 1);      // (a split feed's layer graph: the ramp-merge flavour, when it is on)
        for (size_t bi = 0; bi < c.batches.size(); ++bi) {      // macro steps in order; inside one: gates, projection, FFN up, FFN down of the active layers
            const SwPlan::Batch &b = c.batches[bi];
            if (b.kind == 4) { launch_ramp_latch(ramp_d_, flight_parity_, m, ramp_word_h_, ramp_mode_ != 1 ? 1 : 0, st); continue; }
            timed_begin(cls_of[b.kind]); launch_gemm_z(c.host.data() + b.off, b.n, c.dev + b.off, st); timed_end(cls_of[b.kind]);
            if (b.rn > 0) { timed_begin(T_ROW); launch_row_z(c.rhost.data() + b.roff, b.rn, c.rdev + b.roff, st); timed_end(T_ROW); }
        }
        if (part < 0) lm_stage_proj(m, 0, T, st, ws_);
    }
    if (part < 0 || part == 2) {
        // (split feed: encoder_proj feeds only the search, so it leaves the layer stream with it; its split-K planes, if any, go to
        // a workspace of its own: ws_ belongs to the layers of the next flight by then)
        if (part == 2) lm_stage_proj(m, 0, T, st, ws_sr_);
        hipStream_t keep = search_stream_;
        search_stream_ = st;
        for (int t = 0; t < T; ++t) run_greedy_rounds(m, dump_logits, t, eout_lm_ + (size_t)t * m * d.joiner);
        search_stream_ = keep;
    }
}

int Engine::lm_step(int m, int T, const int *slots, const int *ring_tails, const int *now_ms, float *logits_out, int mode)
{
    const int rows = m * T;
    if (m <= 0 || T <= 0 || rows > cfg_.max_batch || !flight_has_room(rows + m, 1)) { LOGE("engine: layer-major step %d x %d does not fit (max batch %d)", m, T, cfg_.max_batch); abort(); }
    HIP_CHECK(hipSetDevice(cfg_.device));
    const NetDims &d = L_.dims;
    if (!p_lm_) {
        p_lm_ = dmalloc<float>((size_t)cfg_.max_batch * 4 * d.hidden);
        for (int p = 0; p < 2; ++p) eout_lm_buf_[p] = dmalloc<float>((size_t)cfg_.max_batch * d.joiner);
        eout_lm_ = eout_lm_buf_[flight_parity_];
    }
    if (!lm_stream_) {               // the wavefront's stream, events and block bookkeeping (created outside any stream capture)
        HIP_CHECK(hipStreamCreateWithFlags(&lm_stream_, hipStreamNonBlocking));
        for (int i = 0; i < 9; ++i) { hipEvent_t e; HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); lm_events_.push_back(e); }
        for (int i = 0; i < 3; ++i) HIP_CHECK(hipEventCreateWithFlags(&zargs_done_[i], hipEventDisableTiming));
        lm_now_d_ = dmalloc<int>((size_t)cfg_.max_batch); lm_rows_d_ = dmalloc<int>((size_t)cfg_.max_batch); lm_rec_off_d_ = dmalloc<int>(1);
    }
    const int k = stage_step(m, T, slots, ring_tails, now_ms);
    std::lock_guard<std::mutex> cg(capture_mu_);
    mode == 1 ? run_feed_wavefront(m, T, logits_out != nullptr) : run_layer_major(m, T, logits_out != nullptr);
    if (logits_out) read_back_logits(k, rows, logits_out);
    return k;
}

// mode 1: the chunk steps of one feed as a wavefront over the layers (run_sw_chain)
void Engine::run_feed_wavefront(int m, int T, bool dump_logits)
{
    sw_plan(m, T);
    // captured at the SECOND time the shape is seen (by either flight parity), for both parities; until then its launches go out one by one (~0.25 ms of host time)
    const bool graphs = use_graphs_ && !profiling_ && !dump_logits && (sw_graphs_.find(sw_key(m, T)) || sw_graphs_.find(sw_key(m, T, 1)) || sw_graphs_.use(m, T) >= 2);
    // (split: only the FIRST step of a flight: the per-parity buffers keep neighbouring FLIGHTS apart, a second step of the same
    // flight -- a flush runs several -- would have its index fetch and front end overwrite what the first step's layers and
    // search still read; it takes the one-stream path, behind everything the first step put on F and S)
    // (gates clock on: one stream for everything, so that no other stream's kernel shares the CUs with a gates launch while it times itself;
    // the feeds still arrive pipelined, the GPU stays busy and at speed)
    const bool split = graphs && split_streams_ > 0 && overlap_hint_ && flight_steps_ == 1 && !gclk_;
    const hipStream_t on[3] = {split_streams_ >= 2 ? f_stream_ : stream_, stream_, s_stream_};
    if (graphs && !sw_graphs_.find(sw_key(m, T, split ? 1 : 0)))
        capture_both_parities([&]() {
            const SwPlan &pl = sw_plan(m, T);
            if (split) {
                for (int part = 0; part < 3; ++part) cached_graph(sw_graphs_, sw_key(m, T, 1 + part), on[part], [&]() { run_sw_chain(m, T, false, pl, part, on[part]); });
                if (!pl.headless.batches.empty()) cached_graph(sw_graphs_, sw_key(m, T, 4), on[1], [&]() { run_sw_chain(m, T, false, pl, 3, on[1]); });
            } else cached_graph(sw_graphs_, sw_key(m, T), stream_, [&]() { run_sw_chain(m, T, false, pl, -1, stream_); });
        });
    if (split) { launch_split_feed(m, T, on[0]); return; }
    general_prologue();
    if (graphs) { HIP_CHECK(hipGraphLaunch(sw_graphs_.find(sw_key(m, T)), stream_)); return; }
    launch_count_ = 0; run_sw_chain(m, T, dump_logits, sw_plan(m, T), -1, stream_); kernels_per_step_ = (launch_count_ + 1 + T - 1) / T;          // per chunk
}

// split feed: front end on F (`fe`; split_streams_ == 1 keeps it on M), layers on M, search on S, chained by events inside the feed (see "streams" above)
void Engine::launch_split_feed(int m, int T, hipStream_t fe)
{
    settle_pending_layers(true, RampDefer::BY_OTHER);      // (begin_flight has: one deferral at a time)
    if (fe == f_stream_) {
        if (m_unseen_by_f_) { join(f_stream_, stream_); m_unseen_by_f_ = false; }
    } else if (f_unseen_by_m_) { join(stream_, f_stream_); f_unseen_by_m_ = false; }       // (the fbank launch of this flight)
    if (m_unseen_by_s_) { join(s_stream_, stream_); m_unseen_by_s_ = false; }
    PendingFeed pf;
    pf.m = m; pf.T = T; pf.parity = flight_parity_; pf.tr = trace_slot(); pf.hosts = sw_plan(m, T).hosts;
    if (pf.tr) HIP_CHECK(hipEventRecord(pf.tr->ev[0], fe));
    HIP_CHECK(hipGraphLaunch(sw_graphs_.find(sw_key(m, T, 1)), fe));
    if (pf.tr) HIP_CHECK(hipEventRecord(pf.tr->ev[1], fe));
    bool offered = false;
    if (ramp_mode_ != 0) {
        // the feed's front end is through: tell the previous feed's latch (guarded forms: and arm this feed's head).  hostable: that feed's layer graph is still
        // the last thing M was given (m_quiet_, engine.h), and the front end ran beside it on F.  Read before this feed's own enqueues on M.
        // Deferred enqueue: it also needs a latch in that graph -- only a latch reports, and a feed whose graph holds the head unguarded must not be hosted.
        const bool quiet = fe == f_stream_ && m_quiet_.load(std::memory_order_acquire);
        offered = ramp_mode_ == 3 ? quiet : ramp_mode_ == 1 && quiet && m_tail_latch_;
        if (offered) ramp_eligible_.fetch_add(1, std::memory_order_relaxed);
        launch_ramp_ready(ramp_d_, flight_parity_, m, T, offered ? 1 : 0, ramp_mode_ != 1 ? 1 : 0, fe);
        ++ramp_gen_h_;
    }
    if (fe == f_stream_) {          // M waits for the front end: the event is recorded here, behind the ready kernel; the wait is enqueued with the layers
        pf.fe_done = join_ev_[join_pos_++ % join_ev_.size()];
        HIP_CHECK(hipEventRecord(pf.fe_done, f_stream_));
    } else m_unseen_by_f_ = true;   // (front-end kernels on M read ring rows: the next fbank waits for them)
    // ---- deferred enqueue: offered to a chain with a latch, the feed's layer graph waits for that latch's report.  Everything
    // behind the front end -- layers, search, and the record copy and flight event of close_flight() -- is enqueued by settle_pending_layers().
    std::lock_guard<std::mutex> g(defer_mu_);
    const bool defer = ramp_mode_ == 1 && offered;
    if (defer) pend_ = pf;
    const uint64_t word = ramp_word_h_ ? __atomic_load_n(ramp_word_h_, __ATOMIC_ACQUIRE) : 0;
    const bool open = defer_.launch(ramp_gen_h_, defer, word, [&](RampDefer::Flavour f) { enqueue_split_layers(pf, f == RampDefer::HEADLESS); });
    defer_open_.store(open, std::memory_order_release);
}

// (defer_mu_ held, or nothing deferred) the half of a split feed behind its front end: the layer graph on M -- with the head, or headless when the chain in
// front ran the head --, the search on S behind it, and the flight's tail if close_flight() has come in between.  Calls nothing that settles.
void Engine::enqueue_split_layers(const PendingFeed &f, bool headless)
{
    StreamTrace *tr = f.tr;
    auto graph = [&](int part) {
        const hipGraphExec_t g = sw_graphs_.find(GraphCache::Key{f.m, f.T, f.parity * 8 + part});
        if (!g) { LOGE("engine: split feed %d x %d, parity %d: graph %d is missing", f.m, f.T, f.parity, part); abort(); }
        return g;
    };
    if (f.fe_done) { HIP_CHECK(hipStreamWaitEvent(stream_, f.fe_done, 0)); f_unseen_by_m_ = false; }
    if (tr) HIP_CHECK(hipEventRecord(tr->ev[2], stream_));
    HIP_CHECK(hipGraphLaunch(graph(headless ? 4 : 2), stream_));
    if (tr) HIP_CHECK(hipEventRecord(tr->ev[3], stream_));
    if (ramp_mode_ != 0) { m_tail_latch_ = f.hosts; m_quiet_.store(true, std::memory_order_release); }
    join(s_stream_, stream_);
    if (tr) HIP_CHECK(hipEventRecord(tr->ev[4], s_stream_));
    HIP_CHECK(hipGraphLaunch(graph(3), s_stream_));
    if (tr) { HIP_CHECK(hipEventRecord(tr->ev[5], s_stream_)); tr->m = f.m; tr->T = f.T; tr->headless = headless; tr->used = true; }
    s_unseen_by_m_ = true; flight_tail_s_ = true;
    if (f.closed) {
        if (f.pass_bytes) join(s_stream_, f_stream_);
        enqueue_flight_tail(s_stream_, f.parity, f.rec_base, f.rec_pos, f.conf_spans);
    }
}

// ---------------------------------------------------------------- deferred enqueue
// The ONE place a deferred layer graph is enqueued.  Every entry that touches M, S, the flight state or the graph caches comes through here first:
// m_touched() (general_prologue, sync, the uploads, slot zeroing, plan building, captures), sync_streams(), begin_flight, close_flight's readers
// wait_flight / flight_done, the destructor.  wait == false (wait_flight / flight_done: the stepping thread's time between two launches goes there)
// looks at the report once; wait == true polls it.  The report always comes: the chain whose latch writes it is already on M and waits for
// nothing the host still has to enqueue.  Should M run dry without it the books are wrong, and that is fatal rather than a hang.
static inline void cpu_relax()
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#else
    std::this_thread::yield();
#endif
}

bool Engine::settle_pending_layers(bool wait, RampDefer::Who who)
{
    if (!defer_open_.load(std::memory_order_acquire)) return true;
    std::lock_guard<std::mutex> g(defer_mu_);
    if (!defer_.pending()) return true;
    (void)hipSetDevice(cfg_.device);
    bool m_idle = false;
    for (unsigned spins = 0;; ++spins) {
        const uint64_t word = __atomic_load_n(ramp_word_h_, __ATOMIC_ACQUIRE);
        if (defer_.poll(word, who, [&](RampDefer::Flavour f) { enqueue_split_layers(pend_, f == RampDefer::HEADLESS); })) {
            pend_ = PendingFeed();
            defer_open_.store(false, std::memory_order_release);
            return true;
        }
        if (!wait) return false;
        if (m_idle) { LOGE("engine: the layer stream is idle and no latch reported generation %u (word %llx)", defer_.wanted(), (unsigned long long)word); abort(); }
        if ((spins & 1023u) == 1023u) {
            const hipError_t e = hipStreamQuery(stream_);
            if (e == hipSuccess) m_idle = true; else if (e != hipErrorNotReady) HIP_CHECK(e); else (void)hipGetLastError();
        }
        for (int i = 0; i < 16; ++i) cpu_relax();
    }
}

// the flight of this parity is closed and its event is part of what is deferred
bool Engine::deferred_flight(int parity)
{
    std::lock_guard<std::mutex> g(defer_mu_);
    return defer_.pending() && pend_.closed && pend_.parity == parity;
}

void Engine::ramp_defer_counts(uint64_t *headless, uint64_t *by_wait, uint64_t *by_other)
{
    std::lock_guard<std::mutex> g(defer_mu_);
    *headless = defer_.headless; *by_wait = defer_.settled_by[RampDefer::BY_WAIT]; *by_other = defer_.settled_by[RampDefer::BY_OTHER];
}

// mode 0: layer-major; a long feed as a wavefront over blocks of time steps
void Engine::run_layer_major(int m, int T, bool dump_logits)
{
    general_prologue();
    const bool wavefront = lm_wavefront_on() && !profiling_ && T > LM_WAVEFRONT_MIN_CHUNKS &&
                           gemm_plan(args_whr(0, 0, m)).fused && gemm_plan(args_ff2(0, 0, m)).fused;      // (forced, one problem: as the wavefront's forms are built)
    if (wavefront) { run_lm_wavefront(m, T, dump_logits); return; }       // long feed: all layers of a wavefront per launch
    if (!use_graphs_ || profiling_ || dump_logits) { launch_count_ = 0; run_lm_chain(m, T, dump_logits); kernels_per_step_ = launch_count_ + 1; return; }
    const GraphCache::Key key = graph_key(m, T);
    if (!lm_graphs_.find(key) && lm_graphs_.full()) { sync(); lm_graphs_.clear(); }
    HIP_CHECK(hipGraphLaunch(cached_graph(lm_graphs_, key, stream_, [&]() { run_lm_chain(m, T, false); }), stream_));
}

// Stages a step's index block in the flight's pinned ring (read by the advance kernel) and books its records; returns its index inside the flight.
// T == 0: a chunk step, [slots | ring tails | times] of m rows; else the layer-major form: [slots], then ring tails, times and row slots, each [T][m].
int Engine::stage_step(int m, int T, const int *slots, const int *ring_tails, const int *now_ms)
{
    const size_t rows = (size_t)m * (size_t)std::max(T, 1);
    const int k = next_step_index(); int *blk = ring_h_ + ring_pos_;
    memcpy(blk, slots, (size_t)m * 4); memcpy(blk + m, ring_tails, rows * 4); memcpy(blk + m + rows, now_ms, rows * 4);
    for (int t = 0; t < T; ++t) memcpy(blk + m + 2 * rows + (size_t)t * m, slots, (size_t)m * 4);
    step_off_h_[k] = (int)ring_pos_; rec_off_h_[k] = (int)rec_pos_;
    ring_pos_ += (size_t)m + (T ? 3 : 2) * rows; rec_pos_ += 3 * rows;
    if (conf_k_.on()) note_conf_step(k, slots, m, 3 * rows);
    return k;
}

// traced steps (tests): the logits of step k's rounds [3 * rows][vocab] and its records, after everything enqueued has run
void Engine::read_back_logits(int k, int rows, float *out)
{
    const size_t n = (size_t)3 * rows * L_.dims.vocab;
    HIP_CHECK(hipMemcpyAsync(logits_h_, logits_, n * 4, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipMemcpyAsync(rec_h_ + rec_off_h_[k], rec_d_ + rec_off_h_[k], (size_t)3 * rows * sizeof(StepRecord), hipMemcpyDeviceToHost, stream_));
    sync();
    memcpy(out, logits_h_, n * 4);
}

void Engine::drop_graphs()
{
    for (GraphCache *c : {&step_graphs_, &lm_graphs_, &lm_search_graphs_, &sw_graphs_}) c->clear();      // (the feed wavefront plans hold no such pointer: they stay)
}

// ---------------------------------------------------------------- phrase boosting
// The four CSR arrays of a set in ONE device allocation (16-byte aligned parts); the copies are queued on `st`
BiasDesc Engine::upload_bias(const BiasSet &set, void **dev, hipStream_t st)
{
    auto pad = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t ns = set.state_off.size() * 4, ne = std::max<size_t>(set.edge_tok.size(), 1) * 4;
    char *p = nullptr;
    HIP_CHECK(hipMalloc((void **)&p, pad(ns) + 3 * pad(ne)));
    BiasDesc d;
    d.state_off = (const int32_t *)p; d.edge_tok = (const int32_t *)(p + pad(ns)); d.edge_next = (const int32_t *)(p + pad(ns) + pad(ne));
    d.edge_bonus = (const float *)(p + pad(ns) + 2 * pad(ne)); d.n_states = set.states(); d.flags = (int32_t)set.flags;
    HIP_CHECK(hipMemcpyAsync((void *)d.state_off, set.state_off.data(), ns, hipMemcpyHostToDevice, st));
    if (!set.edge_tok.empty()) {
        const size_t b = set.edge_tok.size() * 4;
        HIP_CHECK(hipMemcpyAsync((void *)d.edge_tok, set.edge_tok.data(), b, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync((void *)d.edge_next, set.edge_next.data(), b, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync((void *)d.edge_bonus, set.edge_bonus.data(), b, hipMemcpyHostToDevice, st));
    }
    *dev = p;
    return d;
}

// ---------------------------------------------------------------- slot tables (DESIGN.md sections 12-14)
// Stepping thread, between two flights' enqueues: the queued changes of the three per-slot opt-in tables -> the tables.  The decision
// launches carry the tables (and the side ring) as kernel arguments, null while nobody has opted in: graphs captured until then hold
// the null pointers, so a table's first opt-in drops every captured graph (they are captured again at their next use) after the streams
// have drained -- once per call, however many tables turn on in it.  From then on the pointers never change.  The whole table is
// uploaded, stream-ordered ahead of this flight's steps: the slots that change belong to idle sessions, so no flight in the air reads
// their entries, and the other slots keep their values; a bias set nobody uses any more is read by no flight either.
// LOCK ORDER, here and everywhere: bias_q_.mutex() (the bias books; read_bias_state holds it over its read) -> lm_q_.mutex() (the
// language-model books, likewise; nobody takes the bias mutex under it) -> capture_mu_ -> the
// process-wide legacy-stream lock (step() and the debug entry points take the last two in that order).  The mutexes inside conf_q_ and
// opt_q_ are leaves: held for a push or a take, nothing is locked under them.
void Engine::apply_slot_tables()
{
    std::lock_guard<std::mutex> bg(bias_q_.mutex());
    const auto bias_todo = bias_q_.take_locked();
    std::lock_guard<std::mutex> lg(lm_q_.mutex());
    const auto lm_todo = lm_q_.take_locked();
    const auto conf_todo = conf_q_.take();
    const auto opt_todo = opt_q_.take();
    const size_t S = (size_t)cfg_.max_slots;
    auto in_range = [S](int slot) { return slot >= 0 && (size_t)slot < S; };
    const bool conf_first = !conf_k_.on() && std::any_of(conf_todo.begin(), conf_todo.end(), [](const std::pair<int, int> &t) { return t.second > 0; });
    const bool bias_first = !bias_set_.on() && std::any_of(bias_todo.begin(), bias_todo.end(), [](const std::pair<int, int> &t) { return t.second >= 0; });
    const bool opt_first = !opt_.on() && std::any_of(opt_todo.begin(), opt_todo.end(), [](const std::pair<int, SearchOpt> &t) { return t.second.endpoint_ms != 0; });
    const bool lm_first = !lm_slot_.on() && std::any_of(lm_todo.begin(), lm_todo.end(), [](const std::pair<int, LmSlot> &t) { return t.second.model >= 0; });
    std::lock_guard<std::mutex> cg(capture_mu_);
    if (conf_first || bias_first || opt_first || lm_first) {
        HipLegacyLock legacy;
        sync();
        drop_graphs();
        if (conf_first) {
            conf_k_.alloc(S, 0);
            conf_d_ = dmalloc<ConfRecord>(2 * rec_cap_); conf_h_ = hmalloc<ConfRecord>(2 * rec_cap_);
            LOGI("engine: confidences on (side ring %.0f MB on the device and pinned)", 2.0 * rec_cap_ * sizeof(ConfRecord) / 1e6);
        }
        if (bias_first) {
            bias_set_.alloc(S, -1); bias_desc_.alloc(kBiasSets, BiasDesc()); bias_state_d_ = dmalloc<int32_t>(S);
            LOGI("engine: phrase boosting on");
        }
        if (opt_first) { opt_.alloc(S, SearchOpt{0u, 0.0f}); LOGI("engine: search options on"); }
        if (lm_first) {
            // the LM forms of the decision kernel are built on the BIAS forms: the three bias tables exist from now on as well (every slot: no
            // set; bias_first has allocated them above when a set arrives in the same call)
            if (!bias_set_.on()) {
                bias_set_.alloc(S, -1); bias_desc_.alloc(kBiasSets, BiasDesc()); bias_state_d_ = dmalloc<int32_t>(S);
                HIP_CHECK(hipMemsetAsync(bias_state_d_, 0, S * 4, stream_));
                bias_set_.upload(stream_); bias_desc_.upload(stream_);
            }
            lm_slot_.alloc(S, LmSlot{-1, 0.0f, 0.0f, 0}); lm_desc_.alloc(kLmModels, LmDesc()); lm_state_d_ = dmalloc<int32_t>(S);
            HIP_CHECK(hipMemsetAsync(lm_state_d_, 0, S * 4, stream_));
            LOGI("engine: language models on");
        }
    }
    const bool conf_up = conf_k_.on() && !conf_todo.empty(), bias_up = bias_set_.on() && !bias_todo.empty(), opt_up = opt_.on() && !opt_todo.empty();
    const bool lm_up = lm_slot_.on() && !lm_todo.empty();
    if (!conf_up && !bias_up && !opt_up && !lm_up) return;
    m_touched();
    if (conf_up) {
        for (const auto &t : conf_todo) if (in_range(t.first)) conf_k_.h[t.first] = (uint8_t)t.second;
        conf_k_.upload(stream_);
    }
    if (bias_up) {
        if (bias_first) HIP_CHECK(hipMemsetAsync(bias_state_d_, 0, S * 4, stream_));
        bool sets = false;
        for (int i = 0; i < kBiasSets; ++i) {
            BiasEntry &b = bias_sets_[(size_t)i];
            if (b.set && b.users > 0 && !b.dev) {                     // first use on this engine
                HipLegacyLock legacy;
                bias_desc_.h[i] = upload_bias(*b.set, &b.dev, stream_);
                HIP_CHECK(hipStreamSynchronize(stream_));             // (the source is pageable memory; rare)
                sets = true;
            } else if (b.set && b.users == 0) {                       // the last slot has let go of it
                if (b.dev) { HipLegacyLock legacy; sync_streams(); (void)hipFree(b.dev); b.dev = nullptr; }
                bias_desc_.h[i] = BiasDesc();
                b.set.reset();
                sets = true;
            }
        }
        for (const auto &t : bias_todo) {
            if (!in_range(t.first)) continue;
            bias_set_.h[t.first] = t.second;
            HIP_CHECK(hipMemsetAsync(bias_state_d_ + t.first, 0, 4, stream_));      // every change starts at the root
        }
        if (sets) bias_desc_.upload(stream_);
        bias_set_.upload(stream_);
    }
    if (opt_up) {
        for (const auto &t : opt_todo) if (in_range(t.first)) opt_.h[t.first] = t.second;
        opt_.upload(stream_);
    }
    if (lm_up) {
        bool models = false;
        for (int i = 0; i < kLmModels; ++i) {
            LmEntry &e = lm_models_[(size_t)i];
            if (e.set && e.users > 0 && !e.dev) {                     // first use on this engine
                HipLegacyLock legacy;
                lm_desc_.h[i] = upload_lm(*e.set, &e.dev, stream_);
                HIP_CHECK(hipStreamSynchronize(stream_));             // (the source is pageable memory; rare)
                lm_uploads_.fetch_add(1, std::memory_order_relaxed); lm_resident_.fetch_add(1, std::memory_order_relaxed);
                models = true;
            } else if (e.set && e.users == 0) {                       // the last slot has let go of it
                if (e.dev) { HipLegacyLock legacy; sync_streams(); (void)hipFree(e.dev); e.dev = nullptr; lm_resident_.fetch_sub(1, std::memory_order_relaxed); }
                lm_desc_.h[i] = LmDesc();
                e.set.reset();
                models = true;
            }
        }
        for (const auto &t : lm_todo) {
            if (!in_range(t.first)) continue;
            lm_slot_.h[t.first] = t.second;
            // every change starts at the model's start node (the pinned mirror's entry is the source: it holds this value until the slot's next change)
            HIP_CHECK(hipMemcpyAsync(lm_state_d_ + t.first, &lm_slot_.h[t.first].start, 4, hipMemcpyHostToDevice, stream_));
        }
        if (models) lm_desc_.upload(stream_);
        lm_slot_.upload(stream_);
    }
}

// The eight arrays of a model in ONE device allocation (16-byte aligned parts); the copies are queued on `st`
LmDesc Engine::upload_lm(const LmSet &set, void **dev, hipStream_t st)
{
    auto pad = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t nn = (size_t)set.nodes(), na = std::max<size_t>((size_t)set.arcs(), 1), nt = std::max<size_t>(set.tok_bytes.size(), 1), nv = set.tok_off.size();
    const size_t sz[8] = {pad((nn + 1) * 4), pad(nn * 4), pad(nn * 4), pad(na * 4), pad(na * 4), pad(na), pad(nv * 4), pad(nt)};
    size_t off[9] = {0};
    for (int i = 0; i < 8; ++i) off[i + 1] = off[i] + sz[i];
    char *p = nullptr;
    HIP_CHECK(hipMalloc((void **)&p, off[8]));
    LmDesc d;
    d.node_off = (const int32_t *)(p + off[0]); d.back = (const int32_t *)(p + off[1]); d.bow = (const float *)(p + off[2]);
    d.arc_logp = (const float *)(p + off[3]); d.arc_next = (const int32_t *)(p + off[4]); d.arc_byte = (const uint8_t *)(p + off[5]);
    d.tok_off = (const int32_t *)(p + off[6]); d.tok_bytes = (const uint8_t *)(p + off[7]);
    d.n_nodes = set.nodes(); d.start = set.start; d.unk_logp = set.unk_logp;
    auto put = [&](const void *dst, const void *src, size_t bytes) { if (bytes) HIP_CHECK(hipMemcpyAsync((void *)dst, src, bytes, hipMemcpyHostToDevice, st)); };
    put(d.node_off, set.node_off.data(), (nn + 1) * 4); put(d.back, set.back.data(), nn * 4); put(d.bow, set.bow.data(), nn * 4);
    put(d.arc_logp, set.arc_logp.data(), set.arc_logp.size() * 4); put(d.arc_next, set.arc_next.data(), set.arc_next.size() * 4); put(d.arc_byte, set.arc_byte.data(), set.arc_byte.size());
    put(d.tok_off, set.tok_off.data(), nv * 4); put(d.tok_bytes, set.tok_bytes.data(), set.tok_bytes.size());
    *dev = p;
    return d;
}

int Engine::read_lm_state(int slot)
{
    if (!lm_q_.ever()) return 0;
    std::lock_guard<std::mutex> lg(lm_q_.mutex());        // (apply_slot_tables allocates the table under it)
    if (lm_q_.pending_locked(slot)) { const int i = lm_slot_model_[(size_t)slot]; return i >= 0 ? lm_models_[(size_t)i].set->start : 0; }
    HipLegacyLock legacy;
    HIP_CHECK(hipSetDevice(cfg_.device));
    sync_streams();
    int v = 0;
    if (lm_state_d_) HIP_CHECK(hipMemcpy(&v, lm_state_d_ + slot, 4, hipMemcpyDeviceToHost));
    return v;
}

int Engine::read_bias_state(int slot)
{
    if (!bias_q_.ever()) return 0;
    std::lock_guard<std::mutex> bg(bias_q_.mutex());      // (apply_slot_tables allocates the table under it)
    if (bias_q_.pending_locked(slot)) return 0;
    HipLegacyLock legacy;
    HIP_CHECK(hipSetDevice(cfg_.device));
    sync_streams();
    int v = 0;
    if (bias_state_d_) HIP_CHECK(hipMemcpy(&v, bias_state_d_ + slot, 4, hipMemcpyDeviceToHost));
    return v;
}

void Engine::note_conf_step(int k, const int *slots, int m, size_t records)
{
    bool any = false;
    for (int i = 0; i < m && !any; ++i) any = conf_k_.h[slots[i]] != 0;
    if (!any) return;
    const size_t first = (size_t)rec_off_h_[k];
    if (!conf_spans_.empty() && conf_spans_.back().first + conf_spans_.back().second == first) conf_spans_.back().second += records;
    else conf_spans_.push_back(std::make_pair(first, records));
}

// Flights alternate between the two halves of the per-flight rings, so that the host can enqueue flight k + 1 while the GPU
// still runs flight k and the records of flight k are still being read (Scheduler::loop).  The device step counter starts at
// the half's first step index: the step tables are indexed by it, so the launch chains (graphs) do not depend on the parity.
// the flight's own copies of what the next flight's front end overwrites while this flight's layers / search still read it
void Engine::select_parity(int p)
{
    flight_parity_ = p;
    xb_ = xb_buf_[p]; u_ = u_buf_[p]; ff_ = ff_buf_[p]; xb16_ = xb16_buf_[p]; u16_ = u16_buf_[p]; ff16_ = ff16_buf_[p];
    y_ = y_buf_[p]; ssq_ = ssq_buf_[p]; y16_ = y16_buf_[p]; step_d_ = step_buf_[p]; flags_d_ = flags_buf_[p]; rec_off_d_ = rec_off_buf_[p]; eout_lm_ = eout_lm_buf_[p];
}

void Engine::begin_flight()
{
    HIP_CHECK(hipSetDevice(cfg_.device));
    settle_pending_layers(true, RampDefer::BY_OTHER);
    const int p = flight_parity_ = next_parity_; next_parity_ ^= 1;
    // the buffers of this parity (index ring half, record ring half, y / ssq / step tables, eout_lm) were lent to the flight before the
    // previous one: it must have completed -- the scheduler keeps at most two flights open and completes them in order, so the event
    // is done long ago and this costs nothing; any other caller would silently overwrite an in-flight search
    if (flight_open_[p]) { HIP_CHECK(hipEventSynchronize(flight_done_[p])); flight_open_[p] = false; }
    if (conf_q_.has_pending() || bias_q_.has_pending() || opt_q_.has_pending() || lm_q_.has_pending()) apply_slot_tables();
    conf_spans_.clear();
    ring_base_ = (size_t)p * ring_cap_; rec_base_ = (size_t)p * rec_cap_;
    ring_pos_ = ring_base_; rec_pos_ = rec_base_; flight_steps_ = 0;
    select_parity(p);
    flight_tail_s_ = false;
    { std::lock_guard<std::mutex> g(slot_mu_); zero_pending_slots(); }
}

bool Engine::flight_has_room(int rows, int nsteps) const
{
    // + max_slots: decoder refreshes stage their slot lists in the same index ring
    return flight_steps_ + nsteps <= step_cap_ && ring_pos_ + (size_t)3 * rows + (size_t)cfg_.max_slots <= ring_base_ + ring_cap_ && rec_pos_ + (size_t)3 * rows <= rec_base_ + rec_cap_;
}

int Engine::step(int m, const int *slots, const int *ring_tails, const int *now_ms, float *logits_out)
{
    if (m <= 0 || m > cfg_.max_batch || !flight_has_room(m, 1)) { LOGE("engine: step of %d rows does not fit (max batch %d)", m, cfg_.max_batch); abort(); }
    const int k = stage_step(m, 0, slots, ring_tails, now_ms);
    // The whole per-chunk chain (index fetch + 58 kernels) is replayed from a hipGraph captured once per batch size (and flight
    // parity: the parity selects buffers): at small batches the chain is launch-bound on the host (~3.5 us per launch), the
    // replay is not.  Kernel arguments depend only on m; the step's indices and its record offset reach the kernels through
    // the device step counter.
    std::lock_guard<std::mutex> cg(capture_mu_);               // aas_free on another thread resets slots through this stream
    general_prologue();
    const GraphCache::Key key = graph_key(m);
    if (use_graphs_ && !profiling_ && !logits_out && (step_graphs_.find(key) || step_graphs_.use(m) >= 2)) {      // (captured at the second use, for both parities)
        if (!step_graphs_.find(key)) {
            if (step_graphs_.full()) { sync(); step_graphs_.clear(); }
            capture_both_parities([&]() { cached_graph(step_graphs_, graph_key(m), stream_, [&]() { run_chain(m, false); }); });
        }
        HIP_CHECK(hipGraphLaunch(step_graphs_.find(key), stream_));
        return k;
    }
    launch_count_ = 0; run_chain(m, logits_out != nullptr); kernels_per_step_ = launch_count_ + 1;        // + the index fetch
    if (logits_out) read_back_logits(k, m, logits_out);
    return k;
}

void Engine::decode_rows(int n, const int *slots, int op)
{
    if (n <= 0) return;
    if (dec_table_ && op == 0) return;          // the joiner reads the table row of the slot's context: nothing to refresh
    HIP_CHECK(hipSetDevice(cfg_.device));
    const NetDims &d = L_.dims;
    const int MB = cfg_.max_batch;
    std::lock_guard<std::mutex> cg(capture_mu_);
    general_prologue();
    for (int o = 0; o < n; o += MB) {
        const int m = std::min(MB, n - o);
        if (ring_pos_ + (size_t)m > ring_base_ + ring_cap_) { LOGE("engine: index ring exhausted"); abort(); }
        int *blk = ring_h_ + ring_pos_;                  // staged in the flight's pinned ring: never rewritten before the copy ran
        memcpy(blk, slots + o, (size_t)m * 4);
        ring_pos_ += (size_t)m;
        HIP_CHECK(hipMemcpyAsync(dec_slots_d_, blk, (size_t)m * 4, hipMemcpyHostToDevice, stream_));
        DecRowsArgs a; a.slot_idx = dec_slots_d_; a.M = m; a.op = op; a.blank = P_.blank_id; a.state = gstate_; a.dec = dec_params(); a.de_out = dec_table_ ? nullptr : de_; a.ld_de = d.d_model;
        a.bias_state = bias_state_d_;
        a.lm_slot = lm_slot_.d; a.lm_state = lm_state_d_;
        timed_begin(T_DEC); launch_dec_rows(a, stream_); timed_end(T_DEC);
        if (!dec_table_) run_decproj(m, dec_slots_d_, nullptr, nullptr, 1);
    }
}

int Engine::close_flight()
{
    HIP_CHECK(hipSetDevice(cfg_.device));
    std::lock_guard<std::mutex> cg(capture_mu_);
    settle_pending_layers(false, RampDefer::BY_OTHER);
    {
        // the flight's last step is a split feed whose layers are deferred: its tail is on S behind a search that is not enqueued yet.  The copies and the
        // event go out with it (enqueue_split_layers); wait_flight / flight_done settle before they look at the event.
        std::lock_guard<std::mutex> g(defer_mu_);
        if (defer_.pending()) {
            pend_.closed = true; pend_.pass_bytes = pass_bytes_flight_; pend_.rec_base = rec_base_; pend_.rec_pos = rec_pos_; pend_.conf_spans.swap(conf_spans_);
            pass_bytes_flight_ = false; conf_spans_.clear();
            flight_open_[flight_parity_] = true;
            return flight_parity_;
        }
    }
    // where the flight ends: on S when its last step was a split feed (layers on M, search on S: the record copy must not sit
    // in M's order, where it would hold the next flight's layers back until this search is through), else on M
    hipStream_t tail = s_stream_;
    if (!(flight_tail_s_ && s_unseen_by_m_)) {
        tail = stream_;
        if (f_unseen_by_m_) { join(stream_, f_stream_); f_unseen_by_m_ = false; }
        if (s_unseen_by_m_) { join(stream_, s_stream_); s_unseen_by_m_ = false; }
    } else if (pass_bytes_flight_) join(s_stream_, f_stream_);      // a pass's VAD / DTMF bytes are read after this flight's wait: their copy comes first
    pass_bytes_flight_ = false;
    enqueue_flight_tail(tail, flight_parity_, rec_base_, rec_pos_, conf_spans_);
    conf_spans_.clear();
    flight_open_[flight_parity_] = true;
    return flight_parity_;
}

// the record copy, the side records and the flight's event, at the end of the stream the flight ends on
void Engine::enqueue_flight_tail(hipStream_t tail, int parity, size_t rec_base, size_t rec_pos, const std::vector<std::pair<size_t, size_t>> &conf_spans)
{
    if (rec_pos > rec_base) HIP_CHECK(hipMemcpyAsync(rec_h_ + rec_base, rec_d_ + rec_base, (rec_pos - rec_base) * sizeof(StepRecord), hipMemcpyDeviceToHost, tail));
    for (const auto &sp : conf_spans) {          // side records: only the steps that hold a row of a session with confidences on
        HIP_CHECK(hipMemcpyAsync(conf_h_ + sp.first, conf_d_ + sp.first, sp.second * sizeof(ConfRecord), hipMemcpyDeviceToHost, tail));
        conf_copied_.fetch_add(sp.second, std::memory_order_relaxed);
    }
    HIP_CHECK(hipEventRecord(flight_done_[parity], tail));
}

// (both pollers look at the latch's report alongside the flight's event: this is where the stepping thread is while the hosting chain runs)
bool Engine::flight_done(int parity)
{
    if (!settle_pending_layers(false, RampDefer::BY_WAIT) && deferred_flight(parity)) return false;      // (its event is not recorded yet)
    const hipError_t e = hipEventQuery(flight_done_[parity]);
    if (e == hipSuccess) return true;
    if (e != hipErrorNotReady) HIP_CHECK(e);
    (void)hipGetLastError();
    return false;
}

void Engine::wait_flight(int parity)
{
    HIP_CHECK(hipSetDevice(cfg_.device));
    while (!settle_pending_layers(false, RampDefer::BY_WAIT)) {
        // the deferred flight itself has no event to wait for until it is settled; an older flight may end before the report comes
        if (deferred_flight(parity)) { settle_pending_layers(true, RampDefer::BY_WAIT); break; }
        const hipError_t e = hipEventQuery(flight_done_[parity]);
        if (e == hipSuccess) break;
        if (e != hipErrorNotReady) HIP_CHECK(e);
        (void)hipGetLastError();
        for (int i = 0; i < 16; ++i) cpu_relax();
    }
    HIP_CHECK(hipEventSynchronize(flight_done_[parity]));
    if (profiling_) sync();            // (profiled flights are completed one by one: every launch's event pair has run, collect them)
}

void Engine::end_flight() { wait_flight(close_flight()); }

// ---------------------------------------------------------------- debug / parity entry points
// The debug calls borrow slots 0..n-1; give them back reset (what a new session expects).
void Engine::zero_slots(int n)
{
    const NetDims &d = L_.dims;
    for (int i = 0; i < n; ++i) {
        ZeroSlotArgs z;
        z.h = h_; z.c = c_; z.n_layers = d.n_layers; z.slots = (size_t)cfg_.max_slots; z.d_model = d.d_model; z.hidden = d.hidden;
        z.eout = eout_; z.dout = dout_; z.joiner = d.joiner; z.state = gstate_; z.blank = P_.blank_id; z.slot = i; z.h16 = h16_;
        launch_zero_slot(z, stream_);
    }
    HIP_CHECK(hipStreamSynchronize(stream_));
}

void Engine::debug_encoder(int n, const float *x, const float *h, const float *c, float *eout, float *h2, float *c2)
{
    std::lock_guard<std::mutex> cg(capture_mu_);      // (lock order: apply_slot_tables)
    HipLegacyLock legacy;
    HIP_CHECK(hipSetDevice(cfg_.device));
    const NetDims &d = L_.dims;
    const size_t S = (size_t)cfg_.max_slots;
    if (n > cfg_.max_batch || n > cfg_.max_slots) { LOGE("debug_encoder: n too large"); abort(); }
    // uses slots 0..n-1 directly (callers must not have live sessions); state layout is [n][L][*] on the host
    std::vector<int> slots((size_t)n);
    for (int i = 0; i < n; ++i) slots[(size_t)i] = i;
    float *xd = dmalloc<float>((size_t)n * d.seg * d.mel);
    HIP_CHECK(hipMemcpy(xd, x, (size_t)n * d.seg * d.mel * 4, hipMemcpyHostToDevice));
    for (int i = 0; i < n; ++i)
        for (int l = 0; l < d.n_layers; ++l) {
            HIP_CHECK(hipMemcpy(h_ + ((size_t)l * S + i) * d.d_model, h + ((size_t)i * d.n_layers + l) * d.d_model, (size_t)d.d_model * 4, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(c_ + ((size_t)l * S + i) * d.hidden, c + ((size_t)i * d.n_layers + l) * d.hidden, (size_t)d.hidden * 4, hipMemcpyHostToDevice));
        }
    HIP_CHECK(hipMemcpy(step_d_, slots.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    if (f16_tile_)                              // the binary16 copy of the uploaded h rows (slots 0..n-1 of every layer)
        for (int l = 0; l < d.n_layers; ++l) launch_cvt_f16(h_ + (size_t)l * S * d.d_model, h16_ + (size_t)l * S * d.d_model, (size_t)n * d.d_model, stream_);
    run_encoder_rows(n, xd);
    sync();
    for (int i = 0; i < n; ++i) {
        HIP_CHECK(hipMemcpy(eout + (size_t)i * d.joiner, eout_ + (size_t)i * d.joiner, (size_t)d.joiner * 4, hipMemcpyDeviceToHost));
        for (int l = 0; l < d.n_layers; ++l) {
            HIP_CHECK(hipMemcpy(h2 + ((size_t)i * d.n_layers + l) * d.d_model, h_ + ((size_t)l * S + i) * d.d_model, (size_t)d.d_model * 4, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(c2 + ((size_t)i * d.n_layers + l) * d.hidden, c_ + ((size_t)l * S + i) * d.hidden, (size_t)d.hidden * 4, hipMemcpyDeviceToHost));
        }
    }
    (void)hipFree(xd);
    zero_slots(n);
}

void Engine::debug_decoder(int n, const int64_t *ctx, float *dout)
{
    std::lock_guard<std::mutex> cg(capture_mu_);      // (lock order: apply_slot_tables)
    HipLegacyLock legacy;
    HIP_CHECK(hipSetDevice(cfg_.device));
    const NetDims &d = L_.dims;
    if (n > cfg_.max_batch) { LOGE("debug_decoder: n too large"); abort(); }
    if (dec_table_) {                           // what the sessions read: rows of the table (built by the kernels below, build_dec_table)
        bool in_range = true;
        for (int i = 0; i < n * 2; ++i) if (ctx[i] < 0 || ctx[i] >= d.vocab) in_range = false;
        if (in_range) {
            sync();
            for (int i = 0; i < n; ++i)
                HIP_CHECK(hipMemcpy(dout + (size_t)i * d.joiner, dec_table_ + ((size_t)ctx[2 * i] * d.vocab + (size_t)ctx[2 * i + 1]) * d.joiner, (size_t)d.joiner * 4, hipMemcpyDeviceToHost));
            return;
        }
    }
    std::vector<int> slots((size_t)n), c32((size_t)n * d.context);
    for (int i = 0; i < n; ++i) { slots[(size_t)i] = i; for (int t = 0; t < d.context; ++t) c32[(size_t)i * d.context + t] = (int)ctx[(size_t)i * d.context + t]; }
    int *ctx_d = dmalloc<int>(c32.size());
    HIP_CHECK(hipMemcpy(ctx_d, c32.data(), c32.size() * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dec_slots_d_, slots.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    DecEmbedArgs a; a.dec = dec_params(); a.ctx = ctx_d; a.M = n; a.out = de_; a.ldo = d.d_model;
    launch_dec_embed(a, stream_);
    run_decproj(n, dec_slots_d_, nullptr, nullptr, 1);
    sync();
    HIP_CHECK(hipMemcpy(dout, dout_, (size_t)n * d.joiner * 4, hipMemcpyDeviceToHost));
    (void)hipFree(ctx_d);
    zero_slots(n);
}

void Engine::debug_joiner(int n, const float *eout, const float *dout, float *logits)
{
    std::lock_guard<std::mutex> cg(capture_mu_);      // (lock order: apply_slot_tables)
    HipLegacyLock legacy;
    const NetDims &d = L_.dims;
    HIP_CHECK(hipSetDevice(cfg_.device));
    if (n > cfg_.max_batch) { LOGE("debug_joiner: n too large"); abort(); }
    HIP_CHECK(hipMemcpy(eout_, eout, (size_t)n * d.joiner * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dout_, dout, (size_t)n * d.joiner * 4, hipMemcpyHostToDevice));
    std::vector<int> slots((size_t)n);
    for (int i = 0; i < n; ++i) slots[(size_t)i] = i;
    HIP_CHECK(hipMemcpy(step_d_, slots.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    GemmArgs g; g.a0 = eout_; g.a0b = dout_; g.lda0 = d.joiner; g.aidx0 = step_d_; g.K0 = d.joiner; g.a_op = AOP_TANH_ADD;
    lin(g, L_.w_out); g.M = n; g.N = L_.vocab_pad; g.K = d.joiner; g.kz = kz_out_; g.epi = EPI_PARTIAL; g.out = ws_; g.m_stride = ws_mstride_;
    launch_gemm(g, stream_);
    // logits = tree + bias for all padded columns; the host keeps the first `vocab` of each row
    float *lg = dmalloc<float>((size_t)n * L_.vocab_pad);
    RowArgs r; r.mode = ROW_SLOT_STORE; r.ws = ws_; r.parts = gemm_plan(g).planes; r.m_stride = ws_mstride_; r.N = L_.vocab_pad; r.M = n;
    r.bias = w_ + L_.b_out; r.out = lg; r.ldo = L_.vocab_pad;
    launch_row(r, stream_);
    sync();
    std::vector<float> host((size_t)n * L_.vocab_pad);
    HIP_CHECK(hipMemcpy(host.data(), lg, host.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) memcpy(logits + (size_t)i * d.vocab, host.data() + (size_t)i * L_.vocab_pad, (size_t)d.vocab * 4);
    (void)hipFree(lg);
    zero_slots(n);
}

// slots 0..n-1, row i = slot i; the bias tables and the option table are the call's own
void Engine::debug_decide(const DecideRequest &q)
{
    std::lock_guard<std::mutex> cg(capture_mu_);      // (lock order: apply_slot_tables)
    HipLegacyLock legacy;
    const NetDims &d = L_.dims;
    const int n = q.n;
    HIP_CHECK(hipSetDevice(cfg_.device));
    if (n > cfg_.max_batch || n > cfg_.max_slots) { LOGE("debug_decide: n too large"); abort(); }
    static_assert(sizeof(GreedyState) == 16, "GreedyState is 4 x int32 in the ABI");
    DeviceScratch ds;
    std::vector<int> slots((size_t)n), ones((size_t)n, 1), zeros((size_t)n, 0);
    for (int i = 0; i < n; ++i) slots[(size_t)i] = i;
    const int *slots_d = ds.upload(slots.data(), slots.size());
    if (q.state_io) HIP_CHECK(hipMemcpy(gstate_, q.state_io, (size_t)n * sizeof(GreedyState), hipMemcpyHostToDevice));
    int32_t *bset_d = nullptr, *bstate_d = nullptr; BiasDesc *bdesc_d = nullptr;
    if (q.set) {
        std::vector<int32_t> bset((size_t)n), bstate((size_t)n);
        for (int i = 0; i < n; ++i) { bset[(size_t)i] = q.bias_state_io[i] < 0 ? -1 : 0; bstate[(size_t)i] = std::max(0, q.bias_state_io[i]); }
        void *arrays = nullptr;
        const BiasDesc desc = upload_bias(*q.set, &arrays, stream_);
        ds.adopt(arrays);
        HIP_CHECK(hipStreamSynchronize(stream_));
        bset_d = ds.upload(bset.data(), bset.size()); bstate_d = ds.upload(bstate.data(), bstate.size()); bdesc_d = ds.upload(&desc, 1);
    }
    const SearchOpt *opt_d = q.opts ? ds.upload(q.opts, (size_t)n) : nullptr;
    LmSlot *lslot_d = nullptr; int32_t *lstate_d = nullptr; LmDesc *ldesc_d = nullptr;
    if (q.lm) {      // row i walks the model from node lm_state_io[i], or has none when that is -1
        std::vector<LmSlot> lslot((size_t)n); std::vector<int32_t> lstate((size_t)n);
        for (int i = 0; i < n; ++i) { const bool on = q.lm_state_io[i] >= 0; lslot[(size_t)i] = LmSlot{on ? 0 : -1, on ? q.lm_weight : 0.0f, on ? q.lm_bonus : 0.0f, on ? q.lm->start : 0}; lstate[(size_t)i] = std::max(0, q.lm_state_io[i]); }
        void *arrays = nullptr;
        const LmDesc desc = upload_lm(*q.lm, &arrays, stream_);
        ds.adopt(arrays);
        HIP_CHECK(hipStreamSynchronize(stream_));
        lslot_d = ds.upload(lslot.data(), lslot.size()); lstate_d = ds.upload(lstate.data(), lstate.size()); ldesc_d = ds.upload(&desc, 1);
        if (!q.set) {      // the LM forms are built on the BIAS forms: bias tables in which no row has a set
            std::vector<int32_t> none((size_t)n, -1), root((size_t)n, 0); const BiasDesc empty;
            bset_d = ds.upload(none.data(), none.size()); bstate_d = ds.upload(root.data(), root.size()); bdesc_d = ds.upload(&empty, 1);
        }
    }
    if (q.op == 1) {
        DecRowsArgs a; a.slot_idx = slots_d; a.M = n; a.op = 1; a.blank = P_.blank_id; a.state = gstate_; a.dec = dec_params(); a.de_out = nullptr;
        a.bias_state = bstate_d;
        a.lm_slot = lslot_d; a.lm_state = lstate_d;
        launch_dec_rows(a, stream_);
    } else {
        // the logits enter as ONE partial plane with a zero bias: decide_kernel's tree sum + bias returns them unchanged
        std::vector<float> plane((size_t)n * L_.vocab_pad, -1000.0f);
        for (int i = 0; i < n; ++i) memcpy(plane.data() + (size_t)i * L_.vocab_pad, q.logits + (size_t)i * d.vocab, (size_t)d.vocab * 4);
        StepRecord *rec_d = ds.alloc<StepRecord>((size_t)n);
        ConfRecord *conf_d = q.conf_k > 0 ? ds.zeros<ConfRecord>((size_t)n) : nullptr;
        DecideArgs a;
        a.ws = ds.upload(plane.data(), plane.size()); a.parts = 1; a.m_stride = n; a.N = L_.vocab_pad; a.M = n; a.n_valid = d.vocab;
        a.bias = ds.zeros<float>((size_t)L_.vocab_pad); a.blank = P_.blank_id; a.early_emit = q.early_emit;
        a.slot_idx = slots_d; a.now_ms = ds.upload(q.now_ms ? q.now_ms : zeros.data(), (size_t)n);
        a.active = ds.upload(ones.data(), ones.size());      // every row still searches
        a.dirty = ds.alloc<int>((size_t)n); a.tok_class = cls_; a.state = gstate_;
        a.rec = rec_d; a.round = q.round; a.gen = 1; a.dec = dec_params(); a.de_out = nullptr;
        a.bias_set = bset_d; a.bias_state = bstate_d; a.bias_desc = bdesc_d;
        a.opt = opt_d;
        a.lm_slot = lslot_d; a.lm_state = lstate_d; a.lm_desc = ldesc_d;
        if (conf_d) { a.conf = conf_d; a.conf_k_all = q.conf_k; }
        launch_decide(a, stream_);
        sync();
        if (q.rec_out) HIP_CHECK(hipMemcpy(q.rec_out, rec_d, (size_t)n * sizeof(StepRecord), hipMemcpyDeviceToHost));
        if (conf_d) HIP_CHECK(hipMemcpy(q.conf_out, conf_d, (size_t)n * sizeof(ConfRecord), hipMemcpyDeviceToHost));
    }
    sync();
    if (q.state_io) HIP_CHECK(hipMemcpy(q.state_io, gstate_, (size_t)n * sizeof(GreedyState), hipMemcpyDeviceToHost));
    if (q.set) {
        std::vector<int32_t> bstate((size_t)n);
        HIP_CHECK(hipMemcpy(bstate.data(), bstate_d, (size_t)n * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) if (q.bias_state_io[i] >= 0) q.bias_state_io[i] = bstate[(size_t)i];
    }
    if (q.lm) {
        std::vector<int32_t> lstate((size_t)n);
        HIP_CHECK(hipMemcpy(lstate.data(), lstate_d, (size_t)n * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) if (q.lm_state_io[i] >= 0) q.lm_state_io[i] = lstate[(size_t)i];
    }
    zero_slots(n);
}

void Engine::debug_fbank(int n_frames, const int16_t *pcm_frames, float *out)
{
    // every frame goes to slot 0, consecutive ring rows (n_frames <= ring_frames)
    const int padded = ft_.padded;
    std::vector<FbankFrameDesc> desc((size_t)n_frames);
    for (int i = 0; i < n_frames; ++i) { desc[(size_t)i].slot = 0; desc[(size_t)i].ring_row = i; desc[(size_t)i].pcm_off = i * padded; }
    std::pair<const int16_t *, size_t> part(pcm_frames, (size_t)n_frames * padded);
    fbank(n_frames, desc.data(), &part, 1, (size_t)n_frames * padded);      // (takes capture_mu_ itself: the legacy lock only afterwards, in the same order as step())
    std::lock_guard<std::mutex> cg(capture_mu_);
    HipLegacyLock legacy;
    sync();
    HIP_CHECK(hipMemcpy(out, ring_, (size_t)n_frames * ft_.nbins * 4, hipMemcpyDeviceToHost));
}

void Engine::debug_resample(const ResampleSpec *spec, const int16_t *pcm, size_t n, int16_t *out)
{
    const size_t n_out = (size_t)resample_total((int64_t)n, spec->L, spec->M);
    if (!n_out) return;
    const float *taps = resample_table(spec);
    HipLegacyLock legacy;
    HIP_CHECK(hipSetDevice(cfg_.device));
    DeviceScratch ds;
    int16_t *d = ds.alloc<int16_t>(n + n_out);
    ResampleDesc r;
    r.taps = taps; r.in_base = 0; r.out_first = 0; r.out_end = (int64_t)n_out;
    r.in_off = 0; r.in_n = (int32_t)n; r.out_dst = (int32_t)n; r.out_cnt = (int32_t)n_out;
    r.L = spec->L; r.M = spec->M; r.K = spec->K; r.ldt = spec->ldt;
    if (n) HIP_CHECK(hipMemcpy(d, pcm, n * sizeof(int16_t), hipMemcpyHostToDevice));
    ResampleArgs a;
    a.in = d; a.out = d; a.desc = ds.upload(&r, 1); a.n_desc = 1;
    a.max_blocks = (int)((n_out + kResampleBlock - 1) / kResampleBlock); a.lds_floats = (int)resample_lds_floats(spec->L, spec->M, spec->K);
    run_on_private_stream([&](hipStream_t st) { launch_resample(a, st); });
    HIP_CHECK(hipMemcpy(out, d + n, n_out * sizeof(int16_t), hipMemcpyDeviceToHost));
}

void Engine::debug_decode(uint32_t encoding, uint32_t channels, int32_t channel, const void *data, size_t n_frames, int16_t *out)
{
    if (!n_frames) return;
    const size_t bytes = n_frames * channels * encoding_bytes(encoding);
    HipLegacyLock legacy;
    HIP_CHECK(hipSetDevice(cfg_.device));
    DeviceScratch ds;
    uint8_t *d = ds.alloc<uint8_t>((bytes + 15) / 16 * 16 + n_frames * sizeof(int16_t));      // (hipMalloc: aligned far beyond the contract's 4 bytes)
    DecodeDesc r;
    r.src_off = 0; r.dst = 0; r.out_cnt = r.n_src = (int32_t)n_frames;
    r.encoding = (uint8_t)encoding; r.channels = (uint8_t)channels; r.channel = (int8_t)channel;
    HIP_CHECK(hipMemcpy(d, data, bytes, hipMemcpyHostToDevice));
    DecodeArgs a;
    a.raw = d; a.out = reinterpret_cast<int16_t *>(d + (bytes + 15) / 16 * 16); a.desc = ds.upload(&r, 1); a.n_desc = 1;
    a.max_blocks = (int)((n_frames + kDecodeBlock - 1) / kDecodeBlock);
    run_on_private_stream([&](hipStream_t st) { launch_decode(a, st); });
    HIP_CHECK(hipMemcpy(out, a.out, n_frames * sizeof(int16_t), hipMemcpyDeviceToHost));
}

void Engine::debug_vad(int n_runs, const VadPlan *plans, const int32_t *n, const int32_t *first_row, int ring_rows, const float *rows, VadState *states_io,
                       uint8_t *bytes_out, float *energy_out)
{
    const size_t nb = (size_t)ft_.nbins;
    std::vector<VadDesc> desc((size_t)n_runs);
    std::vector<float> ring((size_t)n_runs * (size_t)ring_rows * nb, 0.0f);
    size_t total = 0;
    for (int r = 0; r < n_runs; ++r) {
        VadDesc &d = desc[(size_t)r];
        d.slot = r; d.first_row = first_row[r]; d.n = n[r]; d.out_off = (int32_t)total; d.plan = plans[r];
        for (int i = 0; i < n[r]; ++i)
            memcpy(&ring[((size_t)r * (size_t)ring_rows + (size_t)((first_row[r] + i) % ring_rows)) * nb], rows + (total + (size_t)i) * nb, nb * sizeof(float));
        total += (size_t)n[r];
    }
    HipLegacyLock legacy;
    HIP_CHECK(hipSetDevice(cfg_.device));
    DeviceScratch ds;
    float *en_d = ds.alloc<float>(total);
    VadState *st_d = ds.upload(states_io, (size_t)n_runs);
    uint8_t *out_d = ds.alloc<uint8_t>(total);
    VadArgs a;
    a.ring = ds.upload(ring.data(), ring.size()); a.ring_frames = ring_rows; a.nbins = ft_.nbins; a.desc = ds.upload(desc.data(), desc.size()); a.n_desc = n_runs;
    a.state = st_d; a.out = out_d; a.energy = en_d;
    run_on_private_stream([&](hipStream_t st) { launch_vad(a, st); });
    HIP_CHECK(hipMemcpy(states_io, st_d, (size_t)n_runs * sizeof(VadState), hipMemcpyDeviceToHost));
    if (total) HIP_CHECK(hipMemcpy(bytes_out, out_d, total, hipMemcpyDeviceToHost));
    if (total && energy_out) HIP_CHECK(hipMemcpy(energy_out, en_d, total * sizeof(float), hipMemcpyDeviceToHost));
}

// The scratch staging the debug entry points of the sample-reading observers share: frame i of the call sits at sample i * padded, as in
// debug_fbank; run r covers the next n[r] frames and writes its records where its frames are.  Fills first / n / out_off of the runs'
// descriptors (the caller has filled the rest) and the args' samples, frame descriptors, descriptors and max_n; returns the frames in all.
template <typename Args, typename Desc>
static size_t debug_stage_runs(Args &a, std::vector<Desc> &desc, const int32_t *n, const int16_t *frames, size_t padded, DeviceScratch &ds)
{
    size_t total = 0;
    for (size_t r = 0; r < desc.size(); ++r) {
        desc[r].first = (int32_t)total; desc[r].n = n[r]; desc[r].out_off = (int32_t)total;
        total += (size_t)n[r]; a.max_n = std::max(a.max_n, n[r]);
    }
    std::vector<FbankFrameDesc> fd(total);
    for (size_t i = 0; i < total; ++i) { fd[i].slot = 0; fd[i].ring_row = 0; fd[i].pcm_off = (int32_t)(i * padded); }
    a.pcm = ds.upload(frames, total * padded); a.frames = ds.upload(fd.data(), fd.size()); a.desc = ds.upload(desc.data(), desc.size()); a.n_desc = (int)desc.size();
    return total;
}

void Engine::debug_dtmf(int n_runs, const DtmfPlan *plans, const int32_t *n, const int16_t *frames, uint8_t *codes_out, float *powers_out)
{
    const float *tables = dtmf_tables();
    std::vector<DtmfDesc> desc((size_t)n_runs);
    for (int r = 0; r < n_runs; ++r) desc[(size_t)r].plan = plans[r];
    HipLegacyLock legacy;
    HIP_CHECK(hipSetDevice(cfg_.device));
    DeviceScratch ds;
    DtmfArgs a;
    const size_t total = debug_stage_runs(a, desc, n, frames, (size_t)ft_.padded, ds);
    a.tables = tables; a.wd = dt_wd_;
    a.out = ds.alloc<uint8_t>(total); a.powers = ds.alloc<float>(total * 9);
    run_on_private_stream([&](hipStream_t st) { launch_dtmf(a, st); });
    HIP_CHECK(hipMemcpy(codes_out, a.out, total, hipMemcpyDeviceToHost));
    if (powers_out) HIP_CHECK(hipMemcpy(powers_out, a.powers, total * 9 * sizeof(float), hipMemcpyDeviceToHost));
}

void Engine::debug_dtmf_decide(const DtmfPlan &plan, int n, const float *powers9, uint8_t *codes_out)
{
    HipLegacyLock legacy;
    HIP_CHECK(hipSetDevice(cfg_.device));
    DeviceScratch ds;
    const float *p = ds.upload(powers9, (size_t)n * 9);
    uint8_t *out = ds.alloc<uint8_t>((size_t)n);
    run_on_private_stream([&](hipStream_t st) { launch_dtmf_decide(plan, n, p, out, st); });
    HIP_CHECK(hipMemcpy(codes_out, out, (size_t)n, hipMemcpyDeviceToHost));
}

void Engine::debug_tones(int n_runs, const TonePlan *plans, const int32_t *n, const int16_t *frames, uint32_t *records_out, float *powers_out)
{
    const float *tables = tone_tables();
    std::vector<ToneDesc> desc((size_t)n_runs);
    for (int r = 0; r < n_runs; ++r) desc[(size_t)r].plan = plans[r];
    const size_t row = (size_t)tn_f_ + 1;
    HipLegacyLock legacy;
    HIP_CHECK(hipSetDevice(cfg_.device));
    DeviceScratch ds;
    ToneArgs a;
    const size_t total = debug_stage_runs(a, desc, n, frames, (size_t)ft_.padded, ds);
    a.tables = tables; a.w = tn_w_; a.f = tn_f_;
    a.out = ds.alloc<uint32_t>(total); a.powers = ds.alloc<float>(total * row);
    run_on_private_stream([&](hipStream_t st) { launch_tone(a, st); });
    HIP_CHECK(hipMemcpy(records_out, a.out, total * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (powers_out) HIP_CHECK(hipMemcpy(powers_out, a.powers, total * row * sizeof(float), hipMemcpyDeviceToHost));
}

void Engine::debug_quality(int hop, int n_runs, const int32_t *clip_levels, const int32_t *n, const int16_t *frames, uint32_t *records_out)
{
    if (hop <= 0 || hop > ft_.padded) { LOGE("a quality hop of %d samples is not inside the frame", hop); abort(); }
    std::vector<QualityDesc> desc((size_t)n_runs);
    for (int r = 0; r < n_runs; ++r) desc[(size_t)r].clip_level = clip_levels[r];
    HipLegacyLock legacy;
    HIP_CHECK(hipSetDevice(cfg_.device));
    DeviceScratch ds;
    QualityArgs a;
    const size_t total = debug_stage_runs(a, desc, n, frames, (size_t)ft_.padded, ds);
    a.hop = hop;
    a.out = ds.alloc<uint32_t>(total * kQualityWords);
    run_on_private_stream([&](hipStream_t st) { launch_quality(a, st); });
    HIP_CHECK(hipMemcpy(records_out, a.out, total * kQualityWords * sizeof(uint32_t), hipMemcpyDeviceToHost));
}

void Engine::debug_tone_decide(const TonePlan &plan, int n, const float *powers, uint32_t *records_out)
{
    HipLegacyLock legacy;
    HIP_CHECK(hipSetDevice(cfg_.device));
    DeviceScratch ds;
    const float *p = ds.upload(powers, (size_t)n * (size_t)(plan.F + 1));
    uint32_t *out = ds.alloc<uint32_t>((size_t)n);
    run_on_private_stream([&](hipStream_t st) { launch_tone_decide(plan, n, p, out, st); });
    HIP_CHECK(hipMemcpy(records_out, out, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
}

void Engine::read_greedy_state(int slot, GreedyState *out)
{
    HipLegacyLock legacy;
    HIP_CHECK(hipSetDevice(cfg_.device));
    sync_streams();
    HIP_CHECK(hipMemcpy(out, gstate_ + slot, sizeof(GreedyState), hipMemcpyDeviceToHost));
}

void Engine::read_ring(int slot, int row, int n_rows, float *out)
{
    HipLegacyLock legacy;
    HIP_CHECK(hipSetDevice(cfg_.device));
    sync_streams();
    const int nb = ft_.nbins;
    for (int i = 0; i < n_rows; ++i)
        HIP_CHECK(hipMemcpy(out + (size_t)i * nb, ring_ + ((size_t)slot * ring_frames_ + (row + i) % ring_frames_) * nb, (size_t)nb * 4, hipMemcpyDeviceToHost));
}

// ---------------------------------------------------------------- snapshot
Engine::SnapLayout Engine::snapshot_layout() const
{
    const NetDims &d = L_.dims;
    SnapLayout l;
    const uint32_t L = (uint32_t)d.n_layers;
    const uint32_t rows[SNAP_ARRAYS] = {L, L, h16_ ? L : 0u, 1u, 1u, 1u, 1u, 1u, 0u};
    const uint32_t bytes[SNAP_ARRAYS] = {(uint32_t)d.d_model * 4u, (uint32_t)d.hidden * 4u, (uint32_t)d.d_model * 2u, (uint32_t)d.joiner * 4u, (uint32_t)d.joiner * 4u,
                                         (uint32_t)sizeof(GreedyState), 4u, (uint32_t)sizeof(VadState), (uint32_t)d.mel * 4u};
    uint32_t off = 0;
    for (int i = 0; i < SNAP_ARRAYS; ++i) {
        l.arr[i].layers = rows[i]; l.arr[i].row_bytes = bytes[i]; l.arr[i].off = off;
        off += (rows[i] * bytes[i] + 15u) / 16u * 16u;
    }
    l.fixed = off;
    return l;
}

// The one body of gather and scatter.  Stepping thread, between flights: the session's flights have completed, and sync() leaves no
// stream with work the copy could overtake; a fresh slot's reset launch is in stream_, the scatter goes behind it on the same stream.
bool Engine::snapshot_copy(int n, SnapRec *recs, uint8_t *const *blocks, bool scatter)
{
    if (n <= 0) return true;
    if (n > 65535) return false;                                   // (grid.y; max_slots is far below)
    HIP_CHECK(hipSetDevice(cfg_.device));
    const NetDims &d = L_.dims;
    const SnapLayout lay = snapshot_layout();
    size_t total = ((size_t)n * sizeof(SnapRec) + 255) / 256 * 256;
    uint32_t max_block = 0;
    bool want_vad = false;
    for (int i = 0; i < n; ++i) {
        SnapRec &r = recs[i];
        const int tail = scatter ? r.tgt_tail : r.tail;
        if (r.slot < 0 || r.slot >= cfg_.max_slots || r.rows < 0 || r.rows > ring_frames_ || tail < 0 || tail >= ring_frames_) return false;
        r.block_bytes = lay.block_bytes(r.rows); r.stage_off = total;
        total += r.block_bytes;
        max_block = std::max(max_block, r.block_bytes);
        want_vad = want_vad || ((r.mask >> SNAP_VAD) & 1u);
    }
    // (the queues first: apply_slot_tables returns a slot with a queued bias change to the root, which must not follow a scatter)
    if (conf_q_.has_pending() || bias_q_.has_pending() || opt_q_.has_pending() || lm_q_.has_pending()) apply_slot_tables();
    std::lock_guard<std::mutex> cg(capture_mu_);
    sync();                                                        // (m_touched() inside: the copy is an enqueue on M like any other)
    if (scatter && want_vad && !vad_state_d_) vad_state_d_ = dmalloc<VadState>((size_t)cfg_.max_slots);
    if (scatter) for (int i = 0; i < n; ++i) if (((recs[i].mask >> SNAP_BIAS) & 1u) && !bias_state_d_) return false;      // (a session with a set: its table exists)
    if (total > snap_cap_) {
        HipLegacyLock legacy;
        if (snap_d_) { HIP_CHECK(hipFree(snap_d_)); HIP_CHECK(hipHostFree(snap_h_)); snap_d_ = snap_h_ = nullptr; }
        snap_cap_ = std::max(total, 2 * snap_cap_);
        snap_d_ = dmalloc<char>(snap_cap_); snap_h_ = hmalloc<char>(snap_cap_);
    }
    SnapArgs a;
    const size_t S = (size_t)cfg_.max_slots;
    char *const base[SNAP_ARRAYS] = {(char *)h_, (char *)c_, (char *)h16_, (char *)eout_, (char *)dout_, (char *)gstate_, (char *)bias_state_d_, (char *)vad_state_d_, (char *)ring_};
    bool wide = ((uintptr_t)snap_d_ % 16) == 0;
    for (int i = 0; i < SNAP_ARRAYS; ++i) {
        SnapArray &x = a.arr[i];
        x.base = base[i]; x.layers = lay.arr[i].layers; x.row_bytes = lay.arr[i].row_bytes; x.off = lay.arr[i].off; x.ring = i == SNAP_RING;
        x.slot_stride = i == SNAP_RING ? (unsigned long long)ring_frames_ * (unsigned long long)d.mel * 4ull : x.row_bytes;
        x.layer_stride = i == SNAP_RING ? x.row_bytes : (unsigned long long)S * x.row_bytes;
        // (the trie state is one word per slot: the kernel moves that word alone, whatever the width of the other accesses)
        if (x.base && (x.layers || x.ring) && x.row_bytes != 4) wide = wide && (uintptr_t)x.base % 16 == 0 && x.slot_stride % 16 == 0 && x.layer_stride % 16 == 0 && x.row_bytes % 16 == 0;
    }
    a.n_arr = SNAP_ARRAYS; a.n = n; a.recs = reinterpret_cast<const SnapRec *>(snap_d_); a.stage = snap_d_; a.ring_frames = ring_frames_;
    a.scatter = scatter ? 1 : 0; a.vec = wide ? 16 : 4; a.max_block = max_block;
    memcpy(snap_h_, recs, (size_t)n * sizeof(SnapRec));
    if (scatter) {
        for (int i = 0; i < n; ++i) memcpy(snap_h_ + recs[i].stage_off, blocks[i], recs[i].block_bytes);
        HIP_CHECK(hipMemcpyAsync(snap_d_, snap_h_, total, hipMemcpyHostToDevice, stream_));
    } else {
        HIP_CHECK(hipMemcpyAsync(snap_d_, snap_h_, (size_t)n * sizeof(SnapRec), hipMemcpyHostToDevice, stream_));
    }
    const int cls = scatter ? T_SNAP_SCATTER : T_SNAP_GATHER;
    timed_begin(cls); launch_snapshot_copy(a, stream_); timed_end(cls);
    if (!scatter) HIP_CHECK(hipMemcpyAsync(snap_h_, snap_d_, total, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    if (profiling_) collect_timing();
    if (!scatter) for (int i = 0; i < n; ++i) memcpy(blocks[i], snap_h_ + recs[i].stage_off, recs[i].block_bytes);
    (scatter ? snap_scatters_ : snap_gathers_).fetch_add(1, std::memory_order_relaxed);
    return true;
}

bool Engine::snapshot_gather(int n, SnapRec *recs, uint8_t *const *blocks_out) { return snapshot_copy(n, recs, blocks_out, false); }
bool Engine::snapshot_scatter(int n, SnapRec *recs, const uint8_t *const *blocks) { return snapshot_copy(n, recs, const_cast<uint8_t *const *>(blocks), true); }

}  // namespace aprilx
