// aprilx_run_gemm (include/aprilx_engine.h): one GEMM launch against host arrays, for tests/test_gpu_gemm_launch.py.  It builds the
// argument block from the description, prepares the binary16 operands with the engine's own kernels and launches the way the engine
// does: a row-epilogue GEMM as Engine::launch_rowepi sends it (gemm_plan; fused as it is, else partial_form + row_form of
// rowepi_forms.h), n > 1 through stage_gemm_z / launch_gemm_z (+ launch_row_z).  No rule of the planner or of a kernel is restated here.
#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>
#include "../../include/aprilx_engine.h"
#include "common.h"
#include "kernels.h"
#include "rowepi_forms.h"
#include "debug_arena.h"

using namespace aprilx;

namespace {

enum { D_N, D_M, D_NC, D_K, D_K0, D_K1, D_KZ, D_EPI, D_AOP, D_WT, D_WAVES, D_TILE_OK, D_FORCE, D_HIDDEN, D_LDO, D_LDA0, D_LDA1, D_LDR, D_LDS, D_LDP,
       D_RUN_FLAG, D_RUN_GEN, D_CTX_VOCAB, D_SAME_B, D_ROWS, D_SLOTS, D_A0_ROWS, D_A1_ROWS, D_A0B_ROWS, D_XG, D_RG, D_OUT, D_OUT16, D_STATE16,
       D_TPIN, D_TPIN_MT, D_TPIN_ZS, D_KPIN, D_KPIN_MT, D_PPIN, D_PPIN_MT };
enum { I_A0, I_A1, I_A0B, I_AIDX0, I_AIDX1, I_AIDX0B, I_SLOT, I_MASK, I_CTX, I_BIAS, I_RESID, I_PADD, I_XSSQ, I_RSSQ, I_CSTATE, I_RESERVED, I_W, N_IN };
enum { O_OUT, O_OUT16, O_STATE, O_STATE16, O_CSTATE, O_SSQ, O_PLANES, N_OUT };
constexpr int MAX_PLANES = 8;

struct Problem {
    GemmArgs g;
    float *planes = nullptr;      // [MAX_PLANES][rows_alloc][N]
    size_t out_rows = 0;
};

}  // namespace

extern "C" int aprilx_run_gemm(const int32_t *d, const float *fd, const void *const *in, void *const *out, int32_t *plan_out)
{
    if (!d || !fd || !in || !out || !plan_out) return -1;
    const int n = d[D_N], M = d[D_M], N = d[D_NC], K = d[D_K];
    const size_t R = (size_t)d[D_ROWS], S = (size_t)d[D_SLOTS];
    if (n < 1 || n > 3 || M < 1 || N < 16 || N % 16 != 0 || K < 64 || K % 64 != 0 || d[D_K0] + d[D_K1] != K) return -1;
    if (R < (size_t)((M + 255) / 256) * 256 || S < 1 || d[D_LDO] < 1 || d[D_LDA0] < d[D_K0] || (d[D_K1] > 0 && d[D_LDA1] < d[D_K1])) return -1;
    const int epi = d[D_EPI];
    const bool row_epi = epi == EPI_HR || epi == EPI_RESID_SSQ || epi == EPI_SLOT_STORE;
    const bool f16 = d[D_WT] == 1, f16_rows = f16 && d[D_TILE_OK] == 2;      // binary16 activation rows: the fp16 tile engines' forms

    Arena A("aprilx_run_gemm");
    hipStream_t st = nullptr;
    int *run_flag = nullptr;
    if (d[D_RUN_FLAG] >= 0) { const int v = d[D_RUN_FLAG]; run_flag = (int *)A.upload(&v, sizeof v, sizeof v); }

    // fp32 rows -> what the kernels read: the same rows, or their binary16 copy (launch_cvt_f16, round to nearest even)
    auto rows_operand = [&](const void *host, size_t rows, size_t ld) -> const float * {
        if (!host) return nullptr;
        const size_t cnt = (rows < R ? R : rows) * ld;
        float *f = (float *)A.upload(host, rows * ld * 4, cnt * 4);
        if (!f16_rows || !f) return f;
        void *h = A.raw(cnt * 2, 0);
        if (h) launch_cvt_f16(f, h, cnt, st);
        return (const float *)h;
    };
    auto ints = [&](const void *host, size_t have, size_t cnt) -> const int * { return host ? (const int *)A.upload(host, have * 4, cnt * 4) : nullptr; };
    auto floats = [&](const void *host, size_t have, size_t cnt) -> float * { return host ? (float *)A.upload(host, have * 4, cnt * 4) : nullptr; };

    std::vector<Problem> P((size_t)n);
    for (int p = 0; p < n; ++p) {
        const void *const *ip = in + (size_t)p * N_IN;
        GemmArgs &g = P[(size_t)p].g;
        if (!ip[I_A0] || !ip[I_W] || (d[D_K1] > 0 && !ip[I_A1])) return -1;
        g.M = M; g.N = N; g.K = K; g.K0 = d[D_K0]; g.K1 = d[D_K1]; g.kz = d[D_KZ]; g.epi = epi; g.a_op = d[D_AOP]; g.wt = d[D_WT]; g.wave_mask = d[D_WAVES];
        g.tile_ok = d[D_TILE_OK]; g.force_fullk = d[D_FORCE]; g.hidden = d[D_HIDDEN]; g.ldo = d[D_LDO]; g.lda0 = d[D_LDA0]; g.lda1 = d[D_LDA1];
        g.ldr = d[D_LDR]; g.ld_state = d[D_LDS]; g.ldp = d[D_LDP]; g.ctx_vocab = d[D_CTX_VOCAB]; g.same_idx_b = d[D_SAME_B]; g.zcount = n;
        g.run_flag = run_flag; g.run_gen = d[D_RUN_GEN];
        g.a0 = rows_operand(ip[I_A0], (size_t)d[D_A0_ROWS], (size_t)g.lda0);
        g.a1 = rows_operand(ip[I_A1], (size_t)d[D_A1_ROWS], (size_t)g.lda1);
        g.a0b = rows_operand(ip[I_A0B], (size_t)d[D_A0B_ROWS], (size_t)g.lda0);
        g.aidx0 = ints(ip[I_AIDX0], (size_t)M, R); g.aidx1 = ints(ip[I_AIDX1], (size_t)M, R); g.aidx0b = ints(ip[I_AIDX0B], (size_t)M, R);
        g.slot_idx = ints(ip[I_SLOT], (size_t)M, R); g.row_mask = ints(ip[I_MASK], (size_t)M, R);
        g.ctx_state = (const GreedyState *)ints(ip[I_CTX], S * 4, S * 4);
        g.bias = floats(ip[I_BIAS], (size_t)N, (size_t)N);
        g.resid = floats(ip[I_RESID], (size_t)M * g.ldr, R * g.ldr);
        g.p_add = floats(ip[I_PADD], (size_t)M * g.ldp, R * g.ldp);
        if (ip[I_XSSQ]) { g.x_scale.ssq = floats(ip[I_XSSQ], (size_t)M * d[D_XG], R * d[D_XG]); g.x_scale.groups = d[D_XG]; g.x_scale.inv_n = fd[0]; g.x_scale.eps = fd[1]; }
        if (ip[I_RSSQ]) { g.r_scale.ssq = floats(ip[I_RSSQ], (size_t)M * d[D_RG], R * d[D_RG]); g.r_scale.groups = d[D_RG]; g.r_scale.inv_n = fd[2]; g.r_scale.eps = fd[3]; }
        // W: x4 packed fp32 as given; binary16 in the same order (launch_cvt_f16) or in the x32 order of the tile engines (launch_repack_x32)
        const size_t wn = (size_t)K * N;
        float *w32 = floats(ip[I_W], wn, wn);
        g.wp = w32;
        if (f16 && w32) {
            void *w16 = A.raw(wn * 2, 0);
            if (w16) { if (f16_rows) launch_repack_x32(w32, w16, K, N, st); else launch_cvt_f16(w32, w16, wn, st); }
            g.wp = w16;
        }
        // outputs: 0xFF over the whole allocation
        size_t &orows = P[(size_t)p].out_rows;
        orows = (epi == EPI_SLOT_STORE && g.slot_idx) ? S : R;
        if (epi == EPI_PARTIAL) {
            P[(size_t)p].planes = (float *)A.raw((size_t)MAX_PLANES * R * N * 4, 0xFF);
            g.out = P[(size_t)p].planes; g.m_stride = (int)R;
        } else {
            if (d[D_OUT]) g.out = (float *)A.raw(orows * g.ldo * 4, 0xFF);
            if (d[D_OUT16]) g.out16 = A.raw(orows * g.ldo * 2, 0xFF);
            if (epi == EPI_HR) {
                g.state = (float *)A.raw(S * g.ld_state * 4, 0xFF);
                if (d[D_STATE16]) g.state16 = A.raw(S * g.ld_state * 2, 0xFF);
            }
            if (epi == EPI_LSTM) { if (!ip[I_CSTATE]) return -1; g.c_state = floats(ip[I_CSTATE], S * g.hidden, S * g.hidden); }
            if (epi == EPI_RESID_SSQ) g.ssq_out = (float *)A.raw(R * (N / SSQ_COLS) * 4, 0xFF);
            if (row_epi) P[(size_t)p].planes = (float *)A.raw((size_t)MAX_PLANES * R * N * 4, 0xFF);
        }
    }
    if (A.bad) return -2;

    gemm_tile_pin(d[D_TPIN], d[D_TPIN_MT], d[D_TPIN_ZS]); gemm_kw_pin(d[D_KPIN], d[D_KPIN_MT]); gemm_pp_pin(d[D_PPIN], d[D_PPIN_MT]);
    struct Unpin { ~Unpin() { gemm_tile_pin(-1, 0, 0); gemm_kw_pin(-1, 0); gemm_pp_pin(-1, 0); } } unpin;

    const GemmQuery q = gemm_query(P[0].g);
    const GemmPlan plan = gemm_plan(P[0].g);
    const bool split = row_epi && !plan.fused;
    const int32_t r[16] = {q.recur_form, q.kw_ok, q.pp_ok, q.pw_ok, plan.route, plan.form, plan.mode, plan.mt, plan.nt, plan.zs, plan.planes, plan.fused, plan.error, split, 0, 0};
    std::memcpy(plan_out, r, sizeof r);
    if (plan.error || plan.planes > MAX_PLANES) return -3;

    if (n == 1) {
        const GemmArgs &f = P[0].g;
        if (!split) launch_gemm(f, st);
        else { launch_gemm(partial_form(f, P[0].planes, (int)R), st); launch_row(row_form(f, P[0].planes, (int)R, plan.planes), st); }
    } else {
        std::vector<GemmArgs> items, staged((size_t)n);
        std::vector<RowArgs> rows;
        for (Problem &pr : P) {
            if (split) { rows.push_back(row_form(pr.g, pr.planes, (int)R, plan.planes)); items.push_back(partial_form(pr.g, pr.planes, (int)R)); }
            else items.push_back(pr.g);
        }
        stage_gemm_z(items.data(), n, staged.data());
        if (split && gemm_plan(staged[0]).planes != plan.planes) return -3;      // (the question and the launch must agree on the planes)
        const GemmArgs *dev = (const GemmArgs *)A.upload(staged.data(), sizeof(GemmArgs) * (size_t)n, sizeof(GemmArgs) * (size_t)n);
        const RowArgs *rdev = split ? (const RowArgs *)A.upload(rows.data(), sizeof(RowArgs) * (size_t)n, sizeof(RowArgs) * (size_t)n) : nullptr;
        if (A.bad) return -2;
        launch_gemm_z(staged.data(), n, dev, st);
        if (split) launch_row_z(rows.data(), n, rdev, st);
    }
    if (!A.ok(hipGetLastError()) || !A.ok(hipDeviceSynchronize())) return -2;

    for (int p = 0; p < n; ++p) {
        void *const *op = out + (size_t)p * N_OUT;
        const Problem &pr = P[(size_t)p];
        const GemmArgs &g = pr.g;
        if (epi != EPI_PARTIAL) { A.download(op[O_OUT], g.out, pr.out_rows * g.ldo * 4); A.download(op[O_OUT16], g.out16, pr.out_rows * g.ldo * 2); }
        A.download(op[O_STATE], g.state, S * g.ld_state * 4); A.download(op[O_STATE16], g.state16, S * g.ld_state * 2);
        A.download(op[O_CSTATE], g.c_state, S * g.hidden * 4);
        A.download(op[O_SSQ], g.ssq_out, R * (N / SSQ_COLS) * 4);
        A.download(op[O_PLANES], pr.planes, (size_t)MAX_PLANES * R * N * 4);
    }
    return A.bad ? -2 : 0;
}
