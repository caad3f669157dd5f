// The GEMM planner (csrc/gemm_plan.h) against the decision table recorded from the planner it replaced
// (tests/golden/gemm_plan_table.npz, exported to a flat int32 file by tests/test_gemm_plan_table_cpu.py), compiled from the header
// alone under AddressSanitizer + UBSan.  Every row, every knob setting and pin combination, all in one process; then the agreement
// between the engine's question and the launch over every row-epilogue row with default knobs.
#include "gemm_plan.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace aprilx;

enum { QCOLS = 26, OCOLS = 9, SCOLS = 18 };
// outputs: kw_before_recur, error, mt, nt, zs, mode, gemm_fullk, gemm_partials (-2: aborts), gemm_tile_planned
enum { O_KWBR, O_ERR, O_MT, O_NT, O_ZS, O_MODE, O_FULLK, O_PARTS, O_TILEP };

static long g_fail = 0, g_checks = 0;
static void fail(const char *what, long row, int setting, long got, long want)
{
    if (++g_fail <= 40) printf("FAIL row %ld setting %d: %s: got %ld, recorded %ld\n", row, setting, what, got, want);
}
#define EXPECT(what, got, want) do { ++g_checks; if ((long)(got) != (long)(want)) fail(what, row, setting, (long)(got), (long)(want)); } while (0)

static GemmQuery query_of(const int32_t *r)
{
    GemmQuery q;
    q.M = r[0]; q.N = r[1]; q.K = r[2]; q.K0 = r[3]; q.K1 = r[4]; q.kz = r[5]; q.epi = r[6]; q.a_op = r[7]; q.wt = r[8]; q.wave_mask = r[9];
    q.has_p_add = r[10] != 0; q.has_x_scale = r[11] != 0; q.zcount = r[12]; q.tile_ok = r[13]; q.force_fullk = r[14];
    q.recur_form = r[22]; q.kw_ok = r[23] != 0; q.pp_ok = r[24] != 0; q.pw_ok = r[25] != 0;      // (the capability bits are part of the recorded row)
    return q;
}
static GemmKnobs knobs_of(const int32_t *s)
{
    GemmKnobs k;
    k.fullk = s[0]; k.gm_tile = s[1]; k.gm_pp = s[2]; k.pp_mt = s[3]; k.pp_wide = s[4]; k.tile_big = s[5]; k.tile_f16_fullk = s[6]; k.gm_kw = s[7]; k.kw_mt = s[8];
    k.kw_over_tile = s[9]; k.z_tiles = s[10];
    k.tile_enable = s[11]; k.tile_pin_mt = s[12]; k.tile_pin_zs = s[13]; k.pp_enable = s[14]; k.pp_pin_mt = s[15]; k.kw_enable = s[16]; k.kw_pin_mt = s[17];
    return k;
}
static bool row_epi(int epi) { return epi == EPI_HR || epi == EPI_RESID_SSQ || epi == EPI_SLOT_STORE; }

static void check_row(long row, int setting, const GemmQuery &q, const GemmKnobs &k, const int32_t *o)
{
    const GemmPlan L = plan_launch(q, k);
    EXPECT("kw_before_recur", kw_before_recur(q, k), o[O_KWBR]);
    EXPECT("stream route", L.route == ROUTE_STREAM, !o[O_KWBR] && q.recur_form);
    if (L.route == ROUTE_STREAM) EXPECT("stream form", L.form, q.recur_form);
    EXPECT("error", L.error, o[O_ERR]);
    if (!o[O_ERR] && !L.error) {
        EXPECT("mt", L.mt, o[O_MT]); EXPECT("nt", L.nt, o[O_NT]); EXPECT("zs", L.zs, o[O_ZS]); EXPECT("mode", L.mode, o[O_MODE]);
        if (L.route != ROUTE_STREAM) {
            const int want = L.mode == GM_PP ? (L.nt == 12 ? ROUTE_PW : ROUTE_PP) : L.mode == GM_TILE ? ROUTE_TILE : L.mode == GM_KW ? ROUTE_KW : ROUTE_KSPLIT;
            EXPECT("route", L.route, want);
        }
    }
    EXPECT("fused (gemm_fullk)", row_fused(q, k), o[O_FULLK]);
    const GemmPlan P = plan_partial_form(q, k);
    if (o[O_PARTS] < 0) EXPECT("partial form error", P.error, PLAN_NO_TILE_PLAN);
    else { EXPECT("partial form error", P.error, PLAN_OK); EXPECT("planes (gemm_partials)", P.planes, o[O_PARTS]); }
    GemmQuery t = q; t.tile_ok = 1;
    EXPECT("gemm_tile_planned", plan_partial_form(t, k).mode == GM_TILE, o[O_TILEP]);
    // the one entry: a row epilogue that is not fused gets its partial form, everything else its launch
    const GemmPlan G = plan_gemm(q, k);
    if (row_epi(q.epi) && !o[O_FULLK]) {
        EXPECT("plan_gemm fused", G.fused, 0);
        if (o[O_PARTS] >= 0) { EXPECT("plan_gemm planes", G.planes, o[O_PARTS]); EXPECT("plan_gemm error", G.error, PLAN_OK); EXPECT("plan_gemm partial mode", G.mode, P.mode); }
    } else {
        EXPECT("plan_gemm route", G.route, L.route); EXPECT("plan_gemm mode", G.mode, L.mode); EXPECT("plan_gemm mt", G.mt, L.mt); EXPECT("plan_gemm nt", G.nt, L.nt);
        EXPECT("plan_gemm zs", G.zs, L.zs); EXPECT("plan_gemm error", G.error, L.error);
        if (row_epi(q.epi) && !L.error) EXPECT("plan_gemm fused", G.fused, 1);
    }
}

// question and launch agree (default knobs): a fused answer launches with all of K however the engine sets force_fullk for the
// launch; a split answer's plane count is what the launch of the partial form writes
static void check_agreement(long row, const GemmQuery &q, const GemmKnobs &k, const int32_t *o)
{
    const int setting = -1;
    if (!row_epi(q.epi) || o[O_ERR] == PLAN_ALWAYS_TILE_OPERANDS || o[O_ERR] == PLAN_NO_TILE_PLAN || o[O_ERR] == PLAN_XSCALE_SHAPE) return;
    const GemmPlan G = plan_gemm(q, k);
    if (G.fused) {
        // launch_rowepi launches with the force it asked with; the z-batched chains ask without and the wavefront with force and
        // launch with 1; an fp16 tile engine's chains launch with 0
        for (int force : {q.force_fullk, 1, 0}) {
            if (force == 0 && q.force_fullk != 0 && !(q.tile_ok == 2 && q.wt == 1)) continue;
            GemmQuery l = q; l.force_fullk = force;
            const GemmPlan p = plan_launch(l, k);
            EXPECT("fused launch error", p.error, PLAN_OK); EXPECT("fused launch zs == kz", p.zs, q.kz);
        }
    } else {
        GemmQuery l = q;      // engine.cc partial_form(): no force, no scales, none of the fused form's kernels
        l.epi = EPI_PARTIAL; l.force_fullk = 0; l.has_x_scale = false; l.recur_form = 0; l.kw_ok = l.pp_ok = l.pw_ok = false;
        const GemmPlan p = plan_launch(l, k);
        EXPECT("partial launch error", p.error, PLAN_OK); EXPECT("partial launch planes", p.planes, G.planes);
    }
}

int main(int argc, char **argv)
{
    if (argc < 2) { printf("usage: gemm_plan_test table.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    int32_t hdr[3];
    if (fread(hdr, 4, 3, f) != 3) return 2;
    const long n = hdr[0], ns = hdr[1], nd = hdr[2];
    std::vector<int32_t> query((size_t)n * QCOLS), def((size_t)n * OCOLS), subset((size_t)n), settings((size_t)ns * SCOLS), dset((size_t)nd), dq((size_t)nd), dout((size_t)nd * OCOLS);
    auto rd = [&](std::vector<int32_t> &v) { return fread(v.data(), 4, v.size(), f) == v.size(); };
    if (!rd(query) || !rd(def) || !rd(subset) || !rd(settings) || !rd(dset) || !rd(dq) || !rd(dout) || fgetc(f) != EOF) { printf("short or long table file\n"); return 2; }
    fclose(f);

    const GemmKnobs defaults;
    long rows_checked = 0, agreement_rows = 0;
    for (long r = 0; r < n; ++r) {
        const GemmQuery q = query_of(&query[(size_t)r * QCOLS]);
        check_row(r, -1, q, defaults, &def[(size_t)r * OCOLS]);
        check_agreement(r, q, defaults, &def[(size_t)r * OCOLS]);
        ++rows_checked; agreement_rows += row_epi(q.epi);
    }
    std::vector<int32_t> want;
    long d = 0;
    for (int s = 0; s < ns; ++s) {
        want = def;
        for (; d < nd && dset[(size_t)d] == s; ++d) {
            if (dq[(size_t)d] < 0 || dq[(size_t)d] >= n) { printf("bad table: diff row out of range\n"); return 2; }
            for (int c = 0; c < OCOLS; ++c) want[(size_t)dq[(size_t)d] * OCOLS + c] = dout[(size_t)d * OCOLS + c];
        }
        const GemmKnobs k = knobs_of(&settings[(size_t)s * SCOLS]);
        for (long r = 0; r < n; ++r) if (subset[(size_t)r]) { check_row(r, s, query_of(&query[(size_t)r * QCOLS]), k, &want[(size_t)r * OCOLS]); ++rows_checked; }
    }
    if (d != nd) { printf("bad table: %ld diff entries left over\n", nd - d); return 2; }
    printf("%ld rows (%ld queries, %ld settings), %ld row-epilogue rows for the agreement, %ld checks, %ld failures\n", rows_checked, n, ns, agreement_rows, g_checks, g_fail);
    if (g_fail || rows_checked == 0) return 1;
    printf("all checks passed\n");
    return 0;
}
