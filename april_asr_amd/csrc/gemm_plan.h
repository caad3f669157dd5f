// Host-side GEMM planning: which schedule, tile and K cut a GEMM runs on, as a pure function of a
// query (plain integers and flags) and of the process's knobs.  Host C++17 only -- no HIP header, no kernels.h -- so that
// tests/cpp/gemm_plan_test.cc compiles it alone.  The schedules themselves are described at the top of kernels.h.
#pragma once
#include <algorithm>

namespace aprilx {

enum GemmEpilogue {
    EPI_PARTIAL = 0,      // ws[z][m][n] = tree sum of this workgroup's slabs      (consumer: row kernels; FULLK: one plane)
    EPI_LSTM = 1,         // columns are unit-major (unit*4 + gate i,f,g,o): cell update, c in place, u out
    EPI_BIAS_DSWISH = 2,  // out = y * sigmoid(y - 1), y = acc + bias
    EPI_HR = 3,           // LSTM projection: state[slot] = acc ; out = resid * rowscale(resid) + acc
    EPI_RESID_SSQ = 4,    // y = resid + (acc + bias) (resid optional) ; out = y ; ssq[m][n/32] = sum of y^2 over 32 columns
    EPI_SLOT_STORE = 5,   // out[slot] = acc + bias, rows with row_mask[m] == 0 skipped (mask optional)
    EPI_XPART = 6         // layer-major schedule: out = (p0 + p1) (* x_scale) = the input half of the gate pre-activations
};
// A-operand prologues
enum GemmAOp { AOP_NONE = 0, AOP_TANH_ADD = 1 };
enum GemmMode { GM_SLAB = 0, GM_FULLK = 1, GM_TILE = 2, GM_KW = 3, GM_PP = 4 };

// The tiles GM_KW is instantiated for (16 mt x 16 nt), stated once: the planner's question and launch_gemm_kw's dispatch
#define APRIL_KW_TILES(X) X(4, 4) X(2, 2) X(1, 2)
inline bool kw_tile_exists(int mt, int nt)
{
#define X(a, b) if (mt == a && nt == b) return true;
    APRIL_KW_TILES(X)
#undef X
    return false;
}

// Everything a plan depends on
struct GemmQuery {
    int M = 0, N = 0, K = 0, K0 = 0, K1 = 0, kz = 1;
    int epi = EPI_PARTIAL, a_op = AOP_NONE, wt = 0, wave_mask = 0xF;
    bool has_p_add = false, has_x_scale = false;
    int zcount = 1;            // same-shape problems sharing the launch
    int tile_ok = 0;           // the caller's: 0 no GM_TILE, 1 by the planner's occupancy rule, 2 always (fp16 tile path)
    int force_fullk = 0;
    // capabilities: what the kernel files say this GEMM can run on (the predicates live beside their geometry constants)
    int recur_form = 0;        // kernels_recur.hip: stream-kernel form 1..6, 0 = none
    bool kw_ok = false;        // kernels_gemm_kw.hip: gemm_kw_waves != 0
    bool pp_ok = false;        // kernels_gemm_pp.hip: gemm_pp_ok(g, 16)
    bool pw_ok = false;        // kernels_gemm_pw.hip: gemm_pw_ok
};

// The process's settings: the environment (filled once, kernels_gemm.hip gemm_knobs) and the bench tools' pins
struct GemmKnobs {
    int fullk = 1;             // APRIL_FULLK
    int gm_tile = 1;           // APRIL_GM_TILE
    int gm_pp = 1;             // APRIL_GM_PP: 0 keeps the round-3 GM_TILE forms
    int pp_mt = 0;             // APRIL_PP_MT: pins the GM_PP tile rows / 16
    int pp_wide = 1;           // APRIL_PP_WIDE: 256 x 192 tiles (kernels_gemm_pw.hip) where they save a round of workgroups
    int tile_big = 1;          // APRIL_TILE_BIG
    int tile_f16_fullk = 1;    // APRIL_TILE_F16_FULLK: 0 restores the cost model's choice (plan_tile)
    int gm_kw = 1;             // APRIL_GM_KW
    int kw_mt = 0;             // APRIL_KW_MT
    int kw_over_tile = 1;      // APRIL_KW_OVER_TILE
    int z_tiles = 2;           // APRIL_Z_TILES, A/B: 0 = plan z-batched problems as if each had the chip to itself, 1 = hint everywhere, 2 = fused-epilogue slab tiles only, 3 = full-K tiles only
    // pins (measurement only): enable -1 = the environment's value, 0 / 1 = off / on; mt, zs = 0 (planner's choice) or pinned
    int tile_enable = -1, tile_pin_mt = 0, tile_pin_zs = 0;      // gemm_tile_pin (tools/tile_bench)
    int pp_enable = -1, pp_pin_mt = 0;                           // gemm_pp_pin (tools/pp_bench)
    int kw_enable = -1, kw_pin_mt = 0;                           // gemm_kw_pin (tools/kw_bench)
};

enum GemmRoute {
    ROUTE_KSPLIT = 0,     // kernels_gemm.hip: GM_SLAB / GM_FULLK
    ROUTE_STREAM = 1,     // kernels_recur.hip, GemmPlan::form
    ROUTE_PP = 2,         // kernels_gemm_pp.hip: 128-column tiles
    ROUTE_PW = 3,         // kernels_gemm_pw.hip: 192-column tiles
    ROUTE_TILE = 4,       // kernels_gemm_tile.hip
    ROUTE_KW = 5          // kernels_gemm_kw.hip
};
enum GemmPlanError {
    PLAN_OK = 0,
    PLAN_ALWAYS_TILE_OPERANDS = 1,   // always-tile GEMM with a prologue / wave mask / odd N
    PLAN_NO_TILE_PLAN = 2,           // no GM_TILE plan for an always-tile GEMM
    PLAN_ROW_NEEDS_FULLK = 3,        // row epilogue without the full-K plan
    PLAN_XSCALE_SHAPE = 4            // x_scale without K0 == K / 2 && kz == 1
};

struct GemmPlan {
    int route = ROUTE_KSPLIT;
    int mode = GM_SLAB, mt = 0, nt = 0, zs = 1;      // (a stream-kernel route carries the plan of the general kernels too: stage_gemm_z stages it)
    int planes = 1;            // partial planes written (1 when fused or GM_FULLK)
    bool fused = false;        // all of K stays in the workgroup
    int form = 0;              // ROUTE_STREAM: the stream-kernel form
    int error = PLAN_OK;       // the launch wrapper prints the message and aborts
};

namespace plan_detail {

struct TilePlan { int mt = 0, nt = 0, zs = 1, mode = GM_SLAB; };

// What plan_tile is asked: a shape and the flags that open its forms
struct TileAsk {
    int M, N, kz, zcount;
    bool force_full;           // no K cut
    bool always;               // fp16 tile engines: every launch size, so that every batch size runs the same chains
    bool big_ok;               // 128 x 128 tiles (fp16 gates / FFN up / XPART)
    bool wide_ok;              // the N = d_model GEMMs of an fp16 tile engine: the "all of K from 192 tiles" rule
    bool pp_ok, pw_ok;         // GM_PP may take it; and its 192-column form
};

inline bool is_slab_epi(int epi) { return epi == EPI_LSTM || epi == EPI_BIAS_DSWISH || epi == EPI_XPART; }
inline bool is_row_epi(int epi) { return epi == EPI_HR || epi == EPI_RESID_SSQ || epi == EPI_SLOT_STORE; }

// The full-K schedule pays once output tiles alone occupy a good part of the chip.  Tiles: at most 64x32 (three
// accumulator-sized register sets: chain, slab, tree level), at least 16x32 (a sum-of-squares granule is 32 columns).
inline bool plan_fullk(int M, int N, int kz, bool force, int zcount, const GemmKnobs &k, TilePlan &t)
{
    constexpr int min_wgs = 96;
    if (!k.fullk || N % 32 != 0) return false;
    const int ncols = N / 32;
    int mt = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
    // (zcount same-shape problems share a launch: the chip is filled by all of them together, so each can use larger tiles)
    while (mt > 1 && (long)ncols * ((M + 16 * mt - 1) / (16 * mt)) * zcount < 256) mt >>= 1;
    const long wgs = (long)ncols * ((M + 16 * mt - 1) / (16 * mt)) * zcount;
    if (wgs < min_wgs && !force) return false;
    t.mt = mt; t.nt = 2; t.zs = kz; t.mode = kz >= 4 ? GM_FULLK : GM_SLAB;    // kz 1 or 2: one workgroup walks the slabs (<= 2 meets)
    return true;
}

// GM_PP (kernels_gemm_pp.hip): the fp16 gates / FFN-up GEMMs on 256 (128) x 128 ping-pong tiles.  One workgroup per CU (144 KB of stage
// buffers), so a launch is ceil(tiles / 256) rounds of one tile time; 256-row tiles are the efficient ones (85 flop per operand byte,
// 16 MFMAs per 8 fragment reads), 128-row tiles fill the chip at fewer rows.  APRIL_GM_PP=0 keeps the round-3 GM_TILE forms;
// APRIL_PP_MT pins the tile rows / 16 (gemm_pp_pin for tools/pp_bench).
inline bool plan_pp(const TileAsk &a, const GemmKnobs &k, TilePlan &t)
{
    constexpr int min_tiles = 128;
    const int M = a.M, N = a.N;
    if (!(k.pp_enable < 0 ? k.gm_pp : k.pp_enable) || N % 128 != 0) return false;
    const long zc = std::max(1, a.zcount);
    const long t16 = (long)(N / 128) * ((M + 255) / 256) * zc, t8 = (long)(N / 128) * ((M + 127) / 128) * zc;
    int mt = k.pp_pin_mt ? k.pp_pin_mt : k.pp_mt;
    int nt = 8;
    if (mt == 12) { if (!a.pw_ok) return false; mt = 16; nt = 12; }      // (pinned: the wide form or nothing)
    else if (mt != 16 && mt != 8) {
        if (t8 < min_tiles) return false;                 // a handful of tiles: the small-batch forms stream the weights with more workgroups
        // rounds of one workgroup per CU; a 128-row tile costs ~0.6 of a 256-row one (half the MFMAs, the same weight pieces), a
        // 256 x 192 tile 1.5 of it: the larger encoder's gates at three 512-row problems are 288 tiles of 256 x 128 (two rounds) but 192
        // of 256 x 192 (one)
        const long c16 = ((t16 + 255) / 256) * 100, c8 = ((t8 + 255) / 256) * 60;
        mt = c16 <= c8 ? 16 : 8;
        if (k.pp_wide && a.pw_ok && N % 192 == 0) {
            const long tw = (long)(N / 192) * ((M + 255) / 256) * zc, cw = ((tw + 255) / 256) * 150;
            if (cw < std::min(c16, c8)) { mt = 16; nt = 12; }
        }
    }
    t.mt = mt; t.nt = nt; t.zs = 1; t.mode = GM_PP;
    return true;
}

// GM_TILE (kernels_gemm_tile.hip): 64-column tiles of 32 (or 64) rows whose waves share the operands through LDS.
// Measured on MI355X (tools/tile_bench, profiles/r03_tile_bench.txt; us per launch, round-2 schedule -> GM_TILE):
//   FFN down 2048 rows x 2 problems 110 -> 83 (32-row tiles, all of K per workgroup), 1024 x 2: 60 -> 46, projection 2048 x 2:
//   64 -> 51, larger encoder 512 x 3: 105 -> 77 (K cut in four, row kernel);  256 rows x 1..3 problems: no gain (a launch of a few
//   hundred short workgroups is bound by its fixed costs -- pipeline fill, the second launch), so small launches keep the
//   round-2 schedules.  Rule: no GM_TILE below 256 32-row tiles per launch; 64-row tiles once the launch holds 512 of them,
//   32-row tiles otherwise; slabs per workgroup from a small cost model (below).
// gemm_tile_pin (tools/tile_bench) pins the choice for measurements.
inline bool plan_tile(const TileAsk &a, const GemmKnobs &k, TilePlan &t)
{
    constexpr int min_rows = 32, fused_tiles = 512, split_tiles = 256;      // (the rule above)
    const int M = a.M, N = a.N, kz = a.kz;
    const int pin_mt = k.tile_pin_mt, pin_zs = k.tile_pin_zs;
    if (N % 64 != 0) return false;
    if (!a.always && (!(k.tile_enable < 0 ? k.gm_tile : k.tile_enable) || M < min_rows)) return false;
    const long zc = std::max(1, a.zcount);
    const long tiles4 = (long)(N / 64) * ((M + 63) / 64) * zc, tiles2 = (long)(N / 64) * ((M + 31) / 32) * zc;
    // (fp16 tile engines: 64-row tiles for the N = d_model GEMMs measured no better than 32-row ones at 512 sessions -- 13.2 vs 12.7 ms
    // of projection + FFN time per 10 feeds -- so the same rule serves both precisions)
    const int mt = pin_mt ? (pin_mt == 4 ? 4 : 2) : (tiles4 >= fused_tiles ? 4 : 2);
    const long tiles = mt == 4 ? tiles4 : tiles2;
    if (a.pp_ok && kz == 1 && pin_mt == 0 && plan_pp(a, k, t)) return true;
    if (a.big_ok && kz == 1 && N % 128 == 0 && pin_mt == 0) {
        // fp16 gates / FFN up: 128 x 128 tiles (eight waves) once they give most CUs a workgroup -- twice the flops per operand byte
        constexpr int big_tiles = 192;
        const long tiles8 = (long)(N / 128) * ((M + 127) / 128) * zc;
        if (k.tile_big && tiles8 >= big_tiles) { t.mt = 8; t.nt = 8; t.zs = 1; t.mode = GM_TILE; return true; }
    }
    int zs = kz;
    // fp16 N = d_model GEMMs (projection, FFN down) keep all of K in the workgroup, i.e. their fused row epilogue: the cost model below
    // prices a K cut at 5 % + 300, but the row kernel behind the planes and its launch boundary cost ~8 us at these sizes -- configs[4]
    // at 512 sessions 1.887 -> 1.820 ms per step with the cut forbidden (round 6; APRIL_TILE_F16_FULLK=0 restores the model's choice)
    // -- from 192 tiles per launch (one 512-row problem); below that the cut is what spreads the weights over the chip
    constexpr int f16_fullk_tiles = 192;
    if (a.always && k.tile_f16_fullk && a.wide_ok && tiles >= f16_fullk_tiles) { }
    else if (pin_zs > 0) { if (!a.force_full) zs = std::min(kz, pin_zs); }
    else if (pin_mt > 0) { /* measurement: pinned tile rows, all of K */ }
    else {
        if (tiles2 < split_tiles && !a.always) return false;          // small launches keep the round-2 schedules
        if (!a.force_full) {
            // workgroups are dealt to the 256 CUs round robin, a CU works through its share at the MFMA rate: cost = (workgroups
            // per CU) x (stages per workgroup + ~3 stages of fill / epilogue), a K cut pays the row kernel on top (~5 %).  A slab is
            // taken as 8 stages (chunks of 4 k blocks); mt = 4 stages hold twice the MFMAs of mt = 2 stages (same for every zs).
            long best = -1;
            for (int z = kz; z >= 1; z >>= 1) {
                const long wgs = tiles * (kz / z), per_cu = (wgs + 255) / 256;
                long cost = per_cu * (8L * z + 3) * 100;
                if (z < kz) cost += cost / 20 + 300;
                if (best < 0 || cost < best) { best = cost; zs = z; }
            }
        }
    }
    t.mt = mt; t.nt = 4; t.zs = zs; t.mode = GM_TILE;
    return true;
}

// Tile shape and slabs per workgroup of the GM_TILE / GM_PP / K-split schedules.  Depends on M only through occupancy; numerics are
// tile-independent.  tile_ok: the effective one; zc_hint: the problem count as the K-split tiles see it; zc: the true one.
inline int plan_tiles(const GemmQuery &q, int epi, bool force_fullk, int tile_ok, int zc_hint, int zc, bool pp_ok, bool pw_ok, const GemmKnobs &k, TilePlan &t)
{
    const int M = q.M, N = q.N, kz = q.kz;
    const bool f16_tile = q.wt == 1 && tile_ok == 2;
    if (tile_ok && (epi == EPI_PARTIAL || is_row_epi(epi) || epi == EPI_LSTM || epi == EPI_BIAS_DSWISH || (epi == EPI_XPART && tile_ok == 2))) {
        TileAsk a;
        a.M = M; a.N = N; a.kz = kz; a.zcount = zc;
        a.force_full = force_fullk || epi != EPI_PARTIAL;      // a row epilogue arrives only when the question's plan kept all of K in the workgroup
        a.always = tile_ok == 2;
        a.big_ok = f16_tile && is_slab_epi(epi);
        a.wide_ok = tile_ok == 2 && (epi == EPI_PARTIAL || epi == EPI_HR || epi == EPI_RESID_SSQ);
        a.pp_ok = f16_tile && pp_ok; a.pw_ok = a.pp_ok && pw_ok;
        if (plan_tile(a, k, t)) return PLAN_OK;
        if (tile_ok == 2) return PLAN_NO_TILE_PLAN;
    }
    if (!is_slab_epi(epi) && plan_fullk(M, N, kz, force_fullk, zc_hint, k, t)) return PLAN_OK;
    const int ntiles = N / 16;
    t.mode = GM_SLAB;
    t.mt = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
    const int mblocks = (M + t.mt * 16 - 1) / (t.mt * 16);
    t.nt = 4;
    // (problems sharing a z-batched launch fill the chip together: wider tiles, i.e. the hand-scheduled 64x32 / 64x64 forms, at
    // fewer rows.  Only for 64-row tiles: the 16-row weight streams of the offline recurrence lose 12 % with 16x64 tiles.)
    const int z = t.mt == 4 ? zc_hint : 1;
    while (t.nt > 1 && ((ntiles % t.nt) != 0 || (long)(ntiles / t.nt) * mblocks * kz * z < 256)) t.nt >>= 1;
    t.zs = 1;
    if (epi == EPI_PARTIAL) {
        // slabs per workgroup grow once the output tiles alone fill the chip; the 64x64 tile has registers for two
        // tree levels only (NLVL in the kernel)
        const long tiles = (long)(ntiles / t.nt) * mblocks;
        const int zs_max = (t.mt == 4 && t.nt == 4) ? 4 : 8;
        while (t.zs < kz && t.zs < zs_max && tiles * (kz / (t.zs * 2)) >= 256) t.zs *= 2;
    }
    return PLAN_OK;
}

constexpr int KW_MIN_ROWS = 3;
inline bool kw_enabled(const GemmKnobs &k) { return (k.kw_enable < 0 ? k.gm_kw : k.kw_enable) != 0; }

// GM_KW (kernels_gemm_kw.hip) takes over a fused full-K plan of the K-split kernels -- the row-epilogue GEMMs on 16..64 x 32
// GM_FULLK / GM_SLAB tiles -- when the operands allow it (kw_ok) and the launch is a few hundred rows: below KW_MIN_ROWS
// the launch is latency-bound either way, above the GM_TILE threshold plan_tile has already taken it.  The decision never changes a
// caller-visible property of the plan (all of K in the workgroup, row work in the epilogue), so the question need not know.
inline void plan_kw(const GemmQuery &q, int zc, const GemmKnobs &k, TilePlan &t)
{
    if (!kw_enabled(k) || t.zs != q.kz) return;
    if (t.mode == GM_TILE) {
        // a FUSED GM_TILE plan (all of K in the workgroup: the same caller-visible shape) keeps the launch unless its tiles fill the 512
        // resident slots badly: half a round or less, or a small remainder behind whole rounds (tools/kw_bench, FFN down: 512 x 2 rows
        // 31.3 (GM_TILE) vs 29.6 us (GM_KW); 768 x 3: 64.8 vs 59.0; 2300 x 2: 117 vs 112; but 1024 x 2: 47 vs 54, 2048 x 3: 123 vs 147)
        if (!k.kw_over_tile || t.nt != 4) return;
        const long tiles = (long)(q.N / 64) * ((q.M + 16 * t.mt - 1) / (16 * t.mt)) * zc;
        const long rem = tiles % 512;
        if (!(tiles <= 256 || (tiles > 512 && rem > 0 && rem <= 128))) return;
    }
    if (q.M < KW_MIN_ROWS || (q.epi != EPI_HR && q.epi != EPI_RESID_SSQ)) return;
    if (!q.kw_ok) return;
    int mt = k.kw_pin_mt ? k.kw_pin_mt : k.kw_mt;
    if (!mt) {
        // 32-row tiles are the efficient ones (one memory instruction per four MFMAs; 16-row tiles: three per eight), 16-row tiles the
        // finer grain: the launch takes ceil(tiles / 256 CUs) rounds, a 16-row round costs ~0.55 of a 32-row one (tools/kw_bench)
        const long t32 = (long)(q.N / 32) * ((q.M + 31) / 32) * zc, t16 = (long)(q.N / 32) * ((q.M + 15) / 16) * zc;
        mt = ((t16 + 255) / 256) * 55 < ((t32 + 255) / 256) * 100 ? 1 : 2;
    }
    const int nt = (mt == 4 && q.N % 64 == 0) ? 4 : 2;      // (pinned 64-row tiles: 64 x 64, a wave tile of one memory instruction per eight MFMAs)
    // APRIL_KW_MT and gemm_kw_pin can ask for shapes that were never instantiated (64-row tiles at N % 64 != 0 ...): the previous plan
    // stays instead of an abort in launch_gemm_kw
    if (!kw_tile_exists(mt, nt)) return;
    t.mt = mt; t.nt = nt; t.zs = q.kz; t.mode = GM_KW;
}

inline void set_plan(GemmPlan &p, const TilePlan &t, int kz)
{
    p.mode = t.mode; p.mt = t.mt; p.nt = t.nt; p.zs = t.zs;
    p.route = t.mode == GM_PP ? (t.nt == 12 ? ROUTE_PW : ROUTE_PP) : t.mode == GM_TILE ? ROUTE_TILE : t.mode == GM_KW ? ROUTE_KW : ROUTE_KSPLIT;
    p.fused = t.zs == kz;
    p.planes = t.mode == GM_FULLK ? 1 : kz / std::max(1, t.zs);
}

}  // namespace plan_detail

// GM_KW instead of the weight-stream row kernel of kernels_recur.hip for the FFN-down GEMM from KW_MIN_ROWS (3) rows:
// 16 x 32 tiles on eight waves against two 16-column tiles on sixteen waves -- 4 / 8 / 16 sessions 0.499 / 0.537 / 0.602 -> 0.475 / 0.496 / 0.527 ms
// per 100 ms feed, one or two rows the same within the noise (they stay on the stream kernels, as does the recurrent pair of a long feed)
inline bool kw_before_recur(const GemmQuery &q, const GemmKnobs &k)
{
    static_assert(plan_detail::KW_MIN_ROWS <= 16, "the row range below is [KW_MIN_ROWS, 16]");
    // (FFN down only: 9.5 .. 12.8 -> 8.2 us per launch at 8 .. 16 rows; the projection's stream kernel is the faster one there, 4.7 .. 5.4 vs 5.8 us)
    return plan_detail::kw_enabled(k) && q.M >= plan_detail::KW_MIN_ROWS && q.M <= 16 && q.epi == EPI_RESID_SSQ && q.kw_ok;
}

// What a launch of exactly this GEMM runs.  Routes in the order they are tried: the stream kernels (unless GM_KW goes first), then
// for tile_ok GEMMs GM_PP (128, then 192 columns), GM_TILE on 128 x 128 tiles, GM_TILE by its rule; else the full-K plan of the
// K-split kernels, else their slab plan; last, GM_KW takes over a fused plan of a few hundred rows.
inline GemmPlan plan_launch(const GemmQuery &q, const GemmKnobs &k)
{
    using namespace plan_detail;
    GemmPlan p;
    if (!kw_before_recur(q, k) && q.recur_form) { p.route = ROUTE_STREAM; p.form = q.recur_form; }
    const int zc = std::max(1, q.zcount);
    const bool slab_epi = is_slab_epi(q.epi);
    // the problem count as the K-split tiles see it (APRIL_Z_TILES); GM_TILE / GM_PP / GM_KW always see the true one
    const int zc_hint = (k.z_tiles == 1 || (k.z_tiles == 2 && slab_epi) || (k.z_tiles == 3 && !slab_epi)) ? zc : 1;
    // GM_TILE eligibility: planner-rule GEMMs (tile_ok 1) are the fp32 row-epilogue / partial GEMMs over one A segment; always-tile
    // GEMMs (tile_ok 2, fp16 tile engines) may also carry two segments and the LSTM / DoubleSwish epilogues
    // (the fp16 tile kernels also have the layer-major halves of the gate GEMM: wave_mask 0x3 + EPI_XPART, 0xC + p_add + EPI_LSTM)
    const bool lm_half = q.tile_ok == 2 && q.wt == 1 && ((q.epi == EPI_XPART && q.wave_mask == 0x3 && !q.has_p_add) || (q.epi == EPI_LSTM && q.wave_mask == 0xC && q.has_p_add));
    const bool plain = q.a_op == AOP_NONE && q.N % 64 == 0 && ((q.wave_mask == 0xF && !q.has_p_add) || lm_half);
    const int tile_ok = !plain ? 0 : (q.tile_ok == 2 ? 2 : ((q.tile_ok == 1 && q.K1 == 0 && q.wt == 0 && q.epi != EPI_LSTM && q.epi != EPI_BIAS_DSWISH) ? 1 : 0));
    if (q.tile_ok == 2 && !tile_ok) { p.error = PLAN_ALWAYS_TILE_OPERANDS; return p; }
    TilePlan t;
    // (any row epilogue forces all of K at launch, whatever `force_fullk` the question was asked with: plan_tiles)
    if ((p.error = plan_tiles(q, q.epi, q.force_fullk != 0, tile_ok, zc_hint, zc, q.wt == 1 && slab_epi && q.pp_ok, q.pw_ok, k, t)) != PLAN_OK) return p;
    plan_kw(q, zc, k, t);
    const int route = p.route;
    set_plan(p, t, q.kz);
    if (route == ROUTE_STREAM) p.route = route;
    if (q.epi != EPI_PARTIAL) p.planes = 1;
    if (is_row_epi(q.epi) && t.zs != q.kz) { p.error = PLAN_ROW_NEEDS_FULLK; return p; }
    // EPI_LSTM with x_scale scales the partial sums of waves 0 and 1: they must hold exactly A segment 0
    if ((q.epi == EPI_LSTM || q.epi == EPI_XPART) && (q.has_x_scale || q.has_p_add || q.wave_mask != 0xF) && (q.kz != 1 || q.K0 * 2 != q.K)) p.error = PLAN_XSCALE_SHAPE;
    return p;
}

// The question a caller asks of a row-epilogue GEMM before it launches it: does its fused form keep all of K in the workgroup?
// Asked with the caller's own tile_ok (not the effective one) and force_fullk.
inline bool row_fused(const GemmQuery &q, const GemmKnobs &k)
{
    using namespace plan_detail;
    TilePlan t;
    // (tile_ok == 2 on a row-epilogue GEMM = the fp16 tile path: its wide tiles take part in the plan, here as at launch)
    const TileAsk a{q.M, q.N, q.kz, q.zcount, q.force_fullk != 0, q.tile_ok == 2, false, q.tile_ok == 2, false, false};
    if (q.tile_ok && plan_tile(a, k, t)) return t.zs == q.kz;
    return plan_fullk(q.M, q.N, q.kz, q.force_fullk != 0, /* not q.zcount: the question never passed it on */ 1, k, t);
}

// The EPI_PARTIAL form of a row-epilogue GEMM, as the question plans it: caller's tile_ok, no force, and the K-split tiles never
// see the problem count (at launch APRIL_Z_TILES 1 / 3 shows it to them).
inline GemmPlan plan_partial_form(const GemmQuery &q, const GemmKnobs &k)
{
    using namespace plan_detail;
    GemmPlan p; TilePlan t;
    GemmQuery f = q; f.wt = 0;      // (the question never knew the operand type: no fp16-only forms)
    if ((p.error = plan_tiles(f, EPI_PARTIAL, false, q.tile_ok, 1, q.zcount, false, false, k, t)) != PLAN_OK) return p;
    set_plan(p, t, q.kz);
    p.fused = false;
    return p;
}

// One plan per GEMM.  A row-epilogue query whose answer is "not fused" gets fused == false, the plan of its EPI_PARTIAL form and
// the planes that form writes; every other query gets what its launch runs.
inline GemmPlan plan_gemm(const GemmQuery &q, const GemmKnobs &k)
{
    if (plan_detail::is_row_epi(q.epi) && !row_fused(q, k)) return plan_partial_form(q, k);
    return plan_launch(q, k);
}

}  // namespace aprilx
