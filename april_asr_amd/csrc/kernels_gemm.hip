// MFMA "skinny" GEMM for gfx950: out[M,N] = A[M,K] x W[K,N], M = sessions
// stepped together (1 .. thousands), W streamed once per workgroup column from a
// pre-packed HBM layout (see kernels.h).  v_mfma_f32_16x16x4_f32 is an exact
// in-order fp32 FMA chain, so results do not depend on M or on the tile shape.
//
// Workgroup = 256 threads = 4 waves which split K; partial tiles meet in LDS and the
// epilogue runs on the summed tile.  Two schedules of the same canonical summation
// (kernels.h): GM_SLAB (waves split every slab, one LDS meet per slab, slabs across
// workgroups -> partial planes; the HBM-bound small-batch form) and GM_FULLK (every wave
// owns a contiguous K quarter, chunk chains and the slab tree are folded in registers,
// ONE LDS meet, no partial planes; the row work runs in the epilogue).  Epilogues:
//   EPI_PARTIAL      slab-tree sums -> workspace (row kernels finish bias/residual/...)
//   EPI_LSTM         LSTM cell: sigma/tanh gates, c' written in place, u = sigma(o) tanh(c')
//   EPI_BIAS_DSWISH  y = acc + b ; y * sigmoid(y - 1)
//   EPI_HR           h state write + residual (LSTM projection)
//   EPI_RESID_SSQ    bias + residual + sum-of-squares partials (BasicNorm is applied by the consumer's A prologue)
//   EPI_SLOT_STORE   bias + store into the session's slot row (encoder_proj, decoder_proj)
// WT = 1 reads fp16 weights and rounds A to fp16 on load (v_mfma_f32_16x16x16_f16, fp32
// accumulation, same lane<->k mapping and summation structure).  The K loop exists twice with
// identical arithmetic: compiler-scheduled C++ (all shapes) and a generated hand-scheduled
// version for the fused-epilogue 64x64 / 64x32 fp32 tiles (gemm_mainloop_asm.inc).
// Replaces the ORT MatMul/Gemm nodes of the encoder/decoder/joiner graphs
// (reference call sites src/april_session.c:145,160,176).
#include "kernels.h"
#include "../../include/aprilx_engine.h"
#include "device_utils.h"
#include "env.h"
// the head of the hand-scheduled K loop on an 8-byte boundary: every instruction of the loop is an 8-byte encoding, so the phase of the
// head is the phase of all of them (MI355X_MICROARCH.md: a hand-written stream loses up to 13 % at shifts of 4 mod 8; the round-5 build
// had the gates kernel's head at 4 mod 8)
#ifndef APRIL_ASM_LOOP_ALIGN
#define APRIL_ASM_LOOP_ALIGN ".p2align 3\n"
#endif
#include "gemm_mainloop_asm.inc"
#ifndef APRIL_ASM_NB
#define APRIL_ASM_NB 2      // operand buffers of the hand-scheduled K loop: 2 keeps two workgroups per CU, 3 needs > 256 registers
#endif
#include <algorithm>
#include <cstdlib>

namespace aprilx {


template <int MT, int NT>
struct TileCfg {
    static constexpr int BM = MT * 16, BN = NT * 16, LDR = BN + 4;
    static constexpr int LDS_FLOATS = 4 * BM * LDR;       // one partial plane per wave; BM row scales follow (LDS_FLOATS + BM floats are requested)
};

template <int WT> struct WQuad { using type = f32x4; };
template <> struct WQuad<1> { using type = h4; };

// ASM = 1: the K loop is the hand-scheduled one (fixed operand registers v112..v175, accumulators in AGPRs); a separate
// instantiation, so that neither loop's registers weigh on the other (both forms must stay within 256 registers: two
// workgroups per CU).  The compiler-scheduled 64-row tiles are told so (second launch-bound = waves per SIMD).
template <int MT, int NT, int EPI, int AOP, int WT, int MODE, int ASM>
__device__ __forceinline__ void gemm_body(const GemmArgs &g, const int zg, const unsigned wg_linear, const int bx, const int by, const bool one_m_block)
{
    using Cfg = TileCfg<MT, NT>;
    constexpr int NW = 4, NTH = NW * 64;                  // waves per workgroup (an eight-wave full-K form measured the same: LAB_NOTES.md)
    using BQ = typename WQuad<WT>::type;       // one lane's four consecutive k values of a weight tile
    extern __shared__ __attribute__((aligned(16))) float red[];
    constexpr bool FULLK = MODE == GM_FULLK;
    constexpr bool ROW_EPI = EPI == EPI_HR || EPI == EPI_RESID_SSQ || EPI == EPI_SLOT_STORE;
    // the slab tree (levels of pairwise sums) is only needed where a workgroup can own more than one slab
    constexpr bool TREE = !FULLK && (EPI == EPI_PARTIAL || ROW_EPI);       // (EPI_LSTM, EPI_BIAS_DSWISH, EPI_XPART: kz = 1)

    if (g.run_flag && *g.run_flag != g.run_gen) return;  // a joiner / decoder round nobody needs (all rows resolved earlier)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // measurement only (tools/gemm_bench built with -DAPRIL_GEMM_TRACE, run with GEMM_TRACE=1): wave 0 stamps s_memtime at
    // phase boundaries (uniform branch, all lanes store the same value); compiled out of the product
#ifdef APRIL_GEMM_TRACE
    auto stamp = [&](int i) { if (g.trace && wave == 0) g.trace[(size_t)wg_linear * 8 + i] = __builtin_amdgcn_s_memtime(); };
#else
    auto stamp = [](int) {};
#endif
    stamp(0);
#ifdef APRIL_GEMM_TRACE
    if (g.trace && wave == 0) {   // where this workgroup runs: HW_ID (wave/simd/cu/sh/se fields) and XCC_ID
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)\n s_getreg_b32 %1, hwreg(HW_REG_XCC_ID)" : "=s"(hw), "=s"(xcc));
        g.trace[(size_t)wg_linear * 8 + 5] = ((unsigned long long)xcc << 32) | hw;
    }
#endif
    // XCD-aware mapping: consecutive blockIdx.x land on different XCDs, so keep the
    // M-blocks that share one weight column on the same XCD (same x mod 8).
    const int nt0 = bx * NT;
    const int m0 = by * Cfg::BM;
    // zg (GM_SLAB): this workgroup owns slabs [zg*zs, (zg+1)*zs)
    const int KB = g.K >> 4;

    const int mrow = lane & 15, kq = lane >> 4;

    // Addressing = uniform 64-bit base (SGPRs; advances with the k block) + one 32-bit byte offset per lane and
    // m-tile (row start + this lane's k quarter), i.e. the saddr form of global_load: no 64-bit vector adds in the loop.
    // All operands are far below 4 GiB per array.
    // after the LDS meet every thread owns QPT groups of 4 consecutive columns ("quads") of the tile
    constexpr int QROW = Cfg::BN / 4, NQ = Cfg::BM * QROW, QPT = (NQ + NTH - 1) / NTH;
    // K blocks: KB = K/16 is a multiple of 4*kz (checked on the host): chunk = c blocks.
    //   GM_SLAB : slab z, wave w -> blocks [(4z + w) c, (4z + w + 1) c); a workgroup walks zs consecutive slabs.
    //   GM_FULLK: wave w of NW -> blocks [w T, (w + 1) T), T = 4 kz c / NW, chunk after chunk (kz / NW whole slabs).
    const int c = g.debug == 1 ? 0 : KB / (4 * g.kz);
    const bool wave_on = ((g.wave_mask >> wave) & 1) != 0;          // layer-major split of the gate GEMM: half of the waves sit a launch out
    const int T = !wave_on ? 0 : (FULLK ? (4 * g.kz / NW) * c : g.zs * c);   // blocks this wave processes in total
    const int first_kb = FULLK ? wave * T : (4 * (zg * g.zs) + wave) * c;

    // BasicNorm scales of the tile's rows, once per workgroup: the rows' sum-of-squares partials make ONE trip from global
    // memory (every lane fetching its own rows' partials cost the gate GEMM 8 us).  The loads are issued here, first thing,
    // and stay in registers during the K loop; after the meet 64 threads add them up through LDS (see the epilogue).
    const RowScale &rsc = EPI == EPI_HR ? g.r_scale : g.x_scale;
    const bool NEED_SCL = (EPI == EPI_HR || EPI == EPI_LSTM || EPI == EPI_SLOT_STORE || EPI == EPI_XPART) && rsc.ssq != nullptr;     // uniform
    float *scl = red + Cfg::LDS_FLOATS;
    float stg[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    // TPR threads share a row, each holds up to 4 consecutive partials of it (no runtime divisions on the way in)
    constexpr int TPR = NTH / Cfg::BM;
    const int ppt = (rsc.groups + TPR - 1) / TPR;
    const bool staged = NEED_SCL && ppt <= 4;
    const int srow = threadIdx.x / TPR, sj0 = (threadIdx.x % TPR) * ppt;
    if (NEED_SCL && staged) {
        int r = m0 + srow;
        if (r >= g.M) r = g.M - 1;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < ppt && sj0 + k < rsc.groups) stg[k] = rsc.ssq[(size_t)r * rsc.groups + sj0 + k];
    }

    // Row indirections (session slots) of all m-tiles are loaded back to back under uniform conditions: ONE memory round trip
    // before the first operand load instead of one per m-tile (the per-tile form compiled to load / s_waitcnt vmcnt(0) four
    // times in a row: ~1.5 us of a 22 us gate GEMM at 256 rows).  Padding rows recompute the last row; never stored.
    uint32_t aoff0[MT], aoff1[MT], aoffb[AOP == AOP_TANH_ADD ? MT : 1];
    int arow[MT], r0v[MT], r1v[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) { const int row = m0 + mt * 16 + mrow; arow[mt] = row >= g.M ? g.M - 1 : row; }
    if (g.aidx0) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) r0v[mt] = g.aidx0[arow[mt]];
    } else {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) r0v[mt] = arow[mt];
    }
    if (g.K1 > 0 && g.aidx1) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) r1v[mt] = g.aidx1[arow[mt]];
    } else {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) r1v[mt] = arow[mt];
    }
    // EPI_LSTM: the slots of this thread's output rows (see below), fetched in the same round trip
    int qslot[EPI == EPI_LSTM ? QPT : 1];
    if (EPI == EPI_LSTM) {
#pragma unroll
        for (int i = 0; i < QPT; ++i) {
            int r = m0 + (int)(threadIdx.x + i * NTH) / QROW;
            if (r >= g.M) r = g.M - 1;
            qslot[i] = g.slot_idx[r];
        }
    }
    if (AOP == AOP_TANH_ADD) {
        int rbv[MT];
        if (g.same_idx_b) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) rbv[mt] = r0v[mt];
        } else if (g.aidx0b) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) rbv[mt] = g.aidx0b[arow[mt]];
        } else {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) rbv[mt] = arow[mt];
        }
        if (g.ctx_state) {
            GreedyState st[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) st[mt] = g.ctx_state[rbv[mt]];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) rbv[mt] = st[mt].ctx0 * g.ctx_vocab + st[mt].ctx1;
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) aoffb[mt] = (uint32_t)(((size_t)rbv[mt] * g.lda0 + kq * 4) * sizeof(float));
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        aoff0[mt] = (uint32_t)(((size_t)r0v[mt] * g.lda0 + kq * 4) * sizeof(float));
        aoff1[mt] = g.K1 > 0 ? (uint32_t)(((size_t)r1v[mt] * g.lda1 + kq * 4) * sizeof(float)) : 0u;
    }
    const uint32_t boff = (uint32_t)lane * sizeof(BQ);
    const bool stream_once = one_m_block;      // weights read by exactly one workgroup: bypass-friendly loads

    // pairwise (balanced-tree) slab accumulation (GM_SLAB): level b holds the sum of 2^b consecutive slabs.  A workgroup
    // that owns zs = 2^t slabs needs t levels; the 64x64 tile is capped at zs = 4 (2 levels, 32 registers) so that it stays
    // within 256 registers and two workgroups share a CU (the planner applies the same cap: gemm_plan.h plan_tiles)
    constexpr int NLVL = !TREE ? 1 : ((MT == 4 && NT == 4) ? 2 : 3);
    f32x4 lvl[NLVL][QPT];
    int top = 0;
    if (TREE) while ((1 << top) < g.zs) ++top;
    constexpr int PLANE = Cfg::BM * Cfg::LDR;
    auto summed4 = [&](int o) {                        // GM_SLAB: ((p0+p1)+p2)+p3 of four consecutive columns; GM_FULLK: balanced tree over the waves' results
        const f32x4 p0 = *reinterpret_cast<const f32x4 *>(red + o), p1 = *reinterpret_cast<const f32x4 *>(red + PLANE + o);
        const f32x4 p2 = *reinterpret_cast<const f32x4 *>(red + 2 * PLANE + o), p3 = *reinterpret_cast<const f32x4 *>(red + 3 * PLANE + o);
        if (FULLK) return (p0 + p1) + (p2 + p3);
        return ((p0 + p1) + p2) + p3;
    };

    auto load_a = [&](int kb, f32x4 (&a)[MT]) {
        const bool seg0 = kb * 16 < g.K0;                    // uniform: segment lengths are multiples of 16
        const char *sb = reinterpret_cast<const char *>(seg0 ? g.a0 : g.a1) + (ptrdiff_t)(seg0 ? kb * 16 : kb * 16 - g.K0) * (ptrdiff_t)sizeof(float);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const uint32_t off = seg0 ? aoff0[mt] : aoff1[mt];
            f32x4 v = *reinterpret_cast<const f32x4 *>(sb + off);
            if (AOP == AOP_TANH_ADD) {
                const f32x4 w = *reinterpret_cast<const f32x4 *>(reinterpret_cast<const char *>(g.a0b) + (ptrdiff_t)kb * 64 + aoffb[mt]);
                v.x = fast_tanh(v.x + w.x); v.y = fast_tanh(v.y + w.y); v.z = fast_tanh(v.z + w.z); v.w = fast_tanh(v.w + w.w);
            }
            a[mt] = v;
        }
    };
    auto load_b = [&](int kb, BQ (&b)[NT]) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const char *sb = reinterpret_cast<const char *>(g.wp) + ((size_t)(nt0 + nt) * KB + kb) * (64 * sizeof(BQ));
            const BQ *pw = reinterpret_cast<const BQ *>(sb + boff);
            b[nt] = stream_once ? __builtin_nontemporal_load(pw) : *pw;
        }
    };

    // Register-staged software pipeline: DEPTH k-blocks of loads are in flight per wave while the MFMAs of the
    // oldest stage issue.  Small batches (MT == 1) are HBM-bound weight streams and want many bytes in flight per
    // CU (6 x 4 waves x (1+NT) KiB); large tiles are MFMA-bound and need only enough depth to cover L2 latency.
    // The prefetch stream runs ahead ACROSS chunk and slab boundaries, so the pipeline never restarts inside a workgroup;
    // loads in the main loop are unconditional (the fetch position parks on the last block) so the loop body is
    // straight-line code and the compiler keeps counted s_waitcnt vmcnt(N) instead of draining.
#ifndef APRIL_DEPTH4
#define APRIL_DEPTH4 2
#endif
    // The full-K tiles are small (16..64 x 32) and read everything through L2: they are bound by bytes in flight per CU
    // (measured 9 TB/s of L2 traffic at 6 stages x 3 KB per wave), so they run deeper.
#ifndef APRIL_FULLK_DEPTH1
#define APRIL_FULLK_DEPTH1 6     // measured: 12 stages are slower (whr 8.7 -> 9.9 us, FFN-down 11.9 -> 13.4 us at 256 rows)
#endif
#ifndef APRIL_DEPTH1
#define APRIL_DEPTH1 6
#endif
#ifndef APRIL_FULLK_DEPTH2
#define APRIL_FULLK_DEPTH2 4
#endif
    constexpr int DEPTH = FULLK ? ((MT == 1) ? APRIL_FULLK_DEPTH1 : (MT == 2 ? APRIL_FULLK_DEPTH2 : 3)) : ((MT == 1) ? APRIL_DEPTH1 : (MT == 2 ? 3 : APRIL_DEPTH4));
    f32x4 a_st[DEPTH][MT];
    BQ b_st[DEPTH][NT];
    int ld_base = first_kb, ld_off = 0, ld_cnt = 0;
    auto ld_next = [&]() {
        const int kb = g.debug == 3 ? 0 : ld_base + ld_off;     // debug 3 (measurement): every block re-reads block 0 (cache-resident operands)
        if (ld_cnt + 1 < T) {
            ++ld_cnt;
            if (FULLK) ++ld_off;                                   // contiguous quarter
            else if (++ld_off == c) { ld_off = 0; ld_base += 4 * c; }
        }
        return kb;
    };
    f32x4 acc[MT][NT];
    auto zero_acc = [&]() {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    auto compute = [&](const f32x4 (&a)[MT], const BQ (&b)[NT]) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const f32x4 av = a[mt];
            if constexpr (WT == 1) {
                // the same 16 k values per lane as four fp32 k-steps, in one v_mfma_f32_16x16x16_f16 (fp32 accumulate)
                const h4 ah = {(_Float16)av.x, (_Float16)av.y, (_Float16)av.z, (_Float16)av.w};
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x16f16(ah, b[nt], acc[mt][nt], 0, 0, 0);
            } else {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, b[nt].x, acc[mt][nt], 0, 0, 0);
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, b[nt].y, acc[mt][nt], 0, 0, 0);
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, b[nt].z, acc[mt][nt], 0, 0, 0);
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, b[nt].w, acc[mt][nt], 0, 0, 0);
                }
            }
        }
    };

    // ---- chunk ends
    // GM_FULLK: the chunk chain is closed in registers.  S = ((c0+c1)+c2)+c3 is a slab; with two slabs per wave (kz = 8)
    // R = S_first + S_second is the first level of the slab tree; the wave's result (a partial tile) is in R.
    f32x4 S[FULLK ? MT : 1][FULLK ? NT : 1], R[FULLK ? MT : 1][FULLK ? NT : 1];
    int chunk_i = 0, slab_i = 0;
    auto fold = [&]() {
        if constexpr (FULLK) {
            if (chunk_i == 0) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) S[mt][nt] = acc[mt][nt];
            } else {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) S[mt][nt] = S[mt][nt] + acc[mt][nt];
            }
            zero_acc();
            if (++chunk_i == 4) {
                chunk_i = 0;
                if (slab_i == 0) {
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) R[mt][nt] = S[mt][nt];
                } else {
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) R[mt][nt] = R[mt][nt] + S[mt][nt];
                }
                ++slab_i;
            }
        }
    };
    // partial tiles -> LDS (red[wave][row][col])
    auto to_lds = [&](const f32x4 (&t)[MT][NT]) {
        float *mine = red + (size_t)wave * PLANE;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    mine[(mt * 16 + kq * 4 + r) * Cfg::LDR + nt * 16 + mrow] = t[mt][nt][r];
            // one m-tile (16 accumulator registers) at a time: left alone, the scheduler copies the whole accumulator
            // file out of the AGPRs first and the kernel no longer fits two workgroups per CU
            if (MT == 4) __builtin_amdgcn_sched_barrier(0);
        }
    };
    int slab_done = 0;                                 // GM_SLAB: slabs finished so far by this workgroup
    f32x4 v[QPT];                                      // this thread's quads of the workgroup's total (valid after the last meet)
    // GM_SLAB: quarter chains meet in LDS and are added ((p0+p1)+p2)+p3; slab sums are combined pairwise in slab order
    // (balanced tree), so owning 1, 2, 4 or 8 slabs per workgroup -- chosen from the batch size -- yields the same bits
    auto meet = [&]() {
        if (slab_done > 0) __syncthreads();            // previous slab's reads of red[] are done
        to_lds(acc);
        __syncthreads();
        if (TREE) {
#pragma unroll
            for (int i = 0; i < QPT; ++i) {
                const int q = threadIdx.x + i * NTH;
                v[i] = q < NQ ? summed4((q / QROW) * Cfg::LDR + (q % QROW) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
            bool carry = true;
#pragma unroll
            for (int b = 0; b < NLVL; ++b) {
                if (carry && b < top) {
                    if ((slab_done >> b) & 1) {
#pragma unroll
                        for (int i = 0; i < QPT; ++i) v[i] = lvl[b][i] + v[i];
                    } else {
#pragma unroll
                        for (int i = 0; i < QPT; ++i) lvl[b][i] = v[i];
                        carry = false;
                    }
                }
            }
        }
        ++slab_done;
    };
    auto chunk_end = [&]() {
        if constexpr (FULLK) fold();
        else { meet(); if (slab_done < g.zs) zero_acc(); }
    };

    // EPI_LSTM: the thread's QPT (row, unit) pairs are known up front; their dependent global loads (row -> slot ->
    // previous cell value) and the gate biases are issued BEFORE the MFMA stream so the epilogue never waits on HBM
    int qm[QPT], qunit[QPT], qo[QPT];
    bool qok[QPT];
    float *cptr[QPT];
    float cprev[QPT];
    f32x4 qb[QPT];
    if (EPI == EPI_LSTM) {
#pragma unroll
        for (int i = 0; i < QPT; ++i) {
            const int q = threadIdx.x + i * NTH;
            const int row = q / QROW, ul = q % QROW;
            qm[i] = m0 + row;
            qok[i] = q < NQ && qm[i] < g.M;
            const int n = nt0 * 16 + ul * 4;
            qunit[i] = n >> 2;
            qo[i] = row * Cfg::LDR + ul * 4;
            cptr[i] = g.c_state + (size_t)qslot[i] * g.hidden + qunit[i];       // (padding rows point at the last row's cell: read, never stored)
            qb[i] = *reinterpret_cast<const f32x4 *>(g.bias + n);
        }
#pragma unroll
        for (int i = 0; i < QPT; ++i) cprev[i] = *cptr[i];
    }

    // Row epilogues: what the epilogue reads besides this kernel's own sums (bias, residual rows, the rows' slots) does not
    // depend on the K loop -- fetched here, into registers, so that the epilogue does not pay two or three dependent L2 round
    // trips after the meet (projection 16x32 at 256 rows: ~1.5 us of 8.7)
    f32x4 e_bias[ROW_EPI ? QPT : 1], e_res[ROW_EPI ? QPT : 1];
    int e_slot[ROW_EPI ? QPT : 1];
    bool e_ok[ROW_EPI ? QPT : 1];
    if (ROW_EPI) {
#pragma unroll
        for (int i = 0; i < QPT; ++i) {
            const int q = threadIdx.x + i * NTH;
            int m = m0 + q / QROW;
            const int n = nt0 * 16 + (q % QROW) * 4;
            e_ok[i] = q < NQ && m < g.M;
            if (m >= g.M) m = g.M - 1;
            const int qn = q < NQ ? n : nt0 * 16;                  // (idle threads of small tiles read a valid column)
            e_slot[i] = (EPI != EPI_RESID_SSQ && g.slot_idx) ? g.slot_idx[m] : m;
            if (EPI == EPI_SLOT_STORE && g.row_mask && !g.row_mask[m]) e_ok[i] = false;
            e_bias[i] = (EPI != EPI_HR) ? *reinterpret_cast<const f32x4 *>(g.bias + qn) : f32x4{0.f, 0.f, 0.f, 0.f};
            e_res[i] = (EPI == EPI_HR || (EPI == EPI_RESID_SSQ && g.resid)) ? *reinterpret_cast<const f32x4 *>(g.resid + (size_t)m * g.ldr + qn) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }

    zero_acc();
    stamp(1);
    // fused-epilogue GEMMs only (one slab, 5..16 blocks per wave): the split-K GEMMs walk several short slabs per
    // workgroup and rely on the cross-slab prefetch of the compiler-scheduled loop below (measured: no gain there)
    if constexpr (ASM) {
        static_assert(!FULLK && MT == 4 && (NT == 4 || NT == 2) && WT == 0 && AOP == AOP_NONE && (EPI == EPI_LSTM || EPI == EPI_BIAS_DSWISH), "no hand-scheduled loop for this form");
        {
            // hand-scheduled K loop (tools/gen_gemm_asm.py): same blocks, same order, same accumulation chains
            uint32_t boffs[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) boffs[nt] = boff + (uint32_t)nt * (uint32_t)KB * 1024u;
            for (int z = 0; z < g.zs; ++z) {
                const int kb0 = (4 * (zg * g.zs + z) + wave) * c;
                int done = wave_on ? 0 : c;
                while (done < c) {
                    const int kb = kb0 + done;
                    const bool seg0 = kb * 16 < g.K0;
                    int n = c - done;
                    if (seg0 && g.K0 / 16 - kb < n) n = g.K0 / 16 - kb;
                    const char *ap = reinterpret_cast<const char *>(seg0 ? g.a0 : g.a1) + (ptrdiff_t)(seg0 ? kb * 16 : kb * 16 - g.K0) * 4;
                    const char *bp = reinterpret_cast<const char *>(g.wp) + ((size_t)nt0 * KB + kb) * 1024;
                    const uint32_t o0 = seg0 ? aoff0[0] : aoff1[0], o1 = seg0 ? aoff0[1] : aoff1[1];
                    const uint32_t o2 = seg0 ? aoff0[2] : aoff1[2], o3 = seg0 ? aoff0[3] : aoff1[3];
#define APRIL_ASM_IN_A [aoff0] "v"(o0), [aoff1] "v"(o1), [aoff2] "v"(o2), [aoff3] "v"(o3), [ap] "s"(ap), [bp] "s"(bp), [nblk] "s"(n)
#define APRIL_ASM_ACC16 [c0] "+a"(acc[0][0]), [c1] "+a"(acc[0][1]), [c2] "+a"(acc[0][2]), [c3] "+a"(acc[0][3]), \
                        [c4] "+a"(acc[1][0]), [c5] "+a"(acc[1][1]), [c6] "+a"(acc[1][2]), [c7] "+a"(acc[1][3]), \
                        [c8] "+a"(acc[2][0]), [c9] "+a"(acc[2][1]), [c10] "+a"(acc[2][2]), [c11] "+a"(acc[2][3]), \
                        [c12] "+a"(acc[3][0]), [c13] "+a"(acc[3][1]), [c14] "+a"(acc[3][2]), [c15] "+a"(acc[3][3])
#define APRIL_ASM_ACC8 [c0] "+a"(acc[0][0]), [c1] "+a"(acc[0][1]), [c2] "+a"(acc[1][0]), [c3] "+a"(acc[1][1]), \
                       [c4] "+a"(acc[2][0]), [c5] "+a"(acc[2][1]), [c6] "+a"(acc[3][0]), [c7] "+a"(acc[3][1])
                    if constexpr (NT == 4) {
                        {
#if APRIL_ASM_NB == 3
                            asm volatile(APRIL_MAINLOOP3_TEXT
#else
                            asm volatile(APRIL_MAINLOOP2_TEXT
#endif
                                : APRIL_ASM_ACC16
                                : APRIL_ASM_IN_A, [boff0] "v"(boffs[0]), [boff1] "v"(boffs[1]), [boff2] "v"(boffs[NT - 2]), [boff3] "v"(boffs[NT - 1])
#if APRIL_ASM_NB == 3
                                : APRIL_MAINLOOP3_CLOBBERS);
#else
                                : APRIL_MAINLOOP2_CLOBBERS);
#endif
                        }
                    } else {
                        {
                            asm volatile(APRIL_MAINLOOP2_NT2_TEXT
                                : APRIL_ASM_ACC8
                                : APRIL_ASM_IN_A, [boff0] "v"(boffs[0]), [boff1] "v"(boffs[1])
                                : APRIL_MAINLOOP2_NT2_CLOBBERS);
                        }
                    }
#undef APRIL_ASM_IN_A
#undef APRIL_ASM_ACC16
#undef APRIL_ASM_ACC8
                    done += n;
                }
                stamp(2);
                meet();
                stamp(3);
                if (slab_done < g.zs) zero_acc();
            }
        }
    }
    else if (T > 0) {
        {
            int first[DEPTH];
#pragma unroll
            for (int s = 0; s < DEPTH; ++s) first[s] = ld_next();
            // same issue order as the steady state (stage by stage, weights then activations): the compiler merges
            // the wait counts of the loop entry and the back edge, and any other order here makes every iteration
            // wait for loads of the NEXT stage (vmcnt(7..4) instead of vmcnt(11..8) at DEPTH 2)
#pragma unroll
            for (int s = 0; s < DEPTH; ++s) {
                load_b(first[s], b_st[s]); load_a(first[s], a_st[s]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        int in_chunk = 0, i = 0;
        for (; i + DEPTH <= T; i += DEPTH) {
#pragma unroll
            for (int s = 0; s < DEPTH; ++s) {
                compute(a_st[s], b_st[s]);
                // pin the refill right behind its stage's MFMAs: left alone, the scheduler sinks all refills to the
                // loop end and the next iteration waits out a full memory latency
                __builtin_amdgcn_sched_barrier(0);
                const int nk = ld_next();
                load_b(nk, b_st[s]); load_a(nk, a_st[s]);
                __builtin_amdgcn_sched_barrier(0);
                if (++in_chunk == c) { in_chunk = 0; chunk_end(); }
            }
        }
#pragma unroll
        for (int s = 0; s < DEPTH - 1; ++s)
            if (i + s < T) {
                compute(a_st[s], b_st[s]);
                if (++in_chunk == c) { in_chunk = 0; chunk_end(); }
            }
    } else {
        if (FULLK) { for (int z = 0; z < 4 * g.kz / NW; ++z) fold(); }
        else for (int z = 0; z < g.zs; ++z) meet();    // measurement mode without the main loop
    }

    if constexpr (!ASM) stamp(2);
    if constexpr (FULLK) {
        // the ONE meet of the full-K schedule: (R0+R1)+(R2+R3) = the canonical slab tree
        to_lds(R);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < QPT; ++i) {
            const int q = threadIdx.x + i * NTH;
            v[i] = q < NQ ? summed4((q / QROW) * Cfg::LDR + (q % QROW) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }

    if (NEED_SCL) {
        // the rows' scales: partials (in registers since the first instruction of the kernel) -> LDS, 64 threads add them in
        // column order (the order of row_scale()); rows are padded to G + 1 floats (conflict-free column walks)
        float *part = scl + Cfg::BM;
        rows_scale_park<Cfg::BM, NTH>(part, rsc, staged, stg, ppt, srow, sj0, m0, g.M, [](const float *p) { return *p; });
        __syncthreads();
        if (threadIdx.x < Cfg::BM) scl[threadIdx.x] = rows_scale_sum(part + threadIdx.x * (rsc.groups + 1), rsc);
        __syncthreads();
    }
    if constexpr (!ASM) stamp(3);
    if (EPI == EPI_PARTIAL) {
#pragma unroll
        for (int i = 0; i < QPT; ++i) {
            const int q = threadIdx.x + i * NTH;
            const int m = m0 + q / QROW;
            if (q < NQ && m < g.M)
                *reinterpret_cast<f32x4 *>(g.out + ((size_t)(FULLK ? 0 : zg) * g.m_stride + m) * g.N + nt0 * 16 + (q % QROW) * 4) = v[i];
        }
    } else if (EPI == EPI_HR) {
        // LSTM projection: h' = acc goes to the session's state row, the layer continues with x + h' where
        // x = y * scale(y) is the (never materialised) BasicNorm output of the previous layer
#pragma unroll
        for (int i = 0; i < QPT; ++i) {
            const int q = threadIdx.x + i * NTH;
            const int m = m0 + q / QROW, n = nt0 * 16 + (q % QROW) * 4;
            if (e_ok[i]) {
                const HrTail t = hr_tail(v[i], e_res[i], scl[q / QROW]);
                *reinterpret_cast<f32x4 *>(g.state + (size_t)e_slot[i] * g.ld_state + n) = t.state;
                *reinterpret_cast<f32x4 *>(g.out + (size_t)m * g.ldo + n) = t.out;
            }
        }
    } else if (EPI == EPI_RESID_SSQ) {
#pragma unroll
        for (int i = 0; i < QPT; ++i) {
            const int q = threadIdx.x + i * NTH;
            const int m = m0 + q / QROW, n = nt0 * 16 + (q % QROW) * 4;
            const bool ok = e_ok[i];
            f32x4 y = f32x4{0.f, 0.f, 0.f, 0.f};
            if (ok) {
                y = resid_tail(v[i], e_bias[i], e_res[i], g.resid != nullptr);
                *reinterpret_cast<f32x4 *>(g.out + (size_t)m * g.ldo + n) = y;
            }
            float ss;                                  // (all lanes take part in the shuffles)
            if (granule_ssq_store(y, ok, q, ss)) g.ssq_out[(size_t)m * (g.N / SSQ_COLS) + n / SSQ_COLS] = ss;
        }
    } else if (EPI == EPI_SLOT_STORE) {
#pragma unroll
        for (int i = 0; i < QPT; ++i) {
            const int q = threadIdx.x + i * NTH;
            const int n = nt0 * 16 + (q % QROW) * 4;
            if (e_ok[i])
                *reinterpret_cast<f32x4 *>(g.out + (size_t)e_slot[i] * g.ldo + n) = NEED_SCL ? slot_value(v[i], scl[q / QROW], e_bias[i]) : slot_value(v[i], e_bias[i]);
        }
    } else if (EPI == EPI_XPART) {
#pragma unroll
        for (int i = 0; i < QPT; ++i) {
            const int q = threadIdx.x + i * NTH;
            const int row = q / QROW, col = (q % QROW) * 4;
            const int m = m0 + row, n = nt0 * 16 + col;
            if (q < NQ && m < g.M) {
                const int o = row * Cfg::LDR + col;
                const f32x4 p0 = *reinterpret_cast<const f32x4 *>(red + o), p1 = *reinterpret_cast<const f32x4 *>(red + PLANE + o);
                *reinterpret_cast<f32x4 *>(g.out + (size_t)m * g.ldo + n) = NEED_SCL ? gate_xin(p0, p1, scl[row]) : (p0 + p1);
            }
        }
    } else if (EPI == EPI_BIAS_DSWISH) {
        // biases of all of this thread's quads first, settled once: a load inside the loop would make every quad wait for the
        // previous quad's store (see EPI_LSTM below)
        f32x4 bq[QPT];
#pragma unroll
        for (int i = 0; i < QPT; ++i) {
            const int q = threadIdx.x + i * NTH;
            bq[i] = *reinterpret_cast<const f32x4 *>(g.bias + nt0 * 16 + (q < NQ ? (q % QROW) * 4 : 0));
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0)
#pragma unroll
        for (int i = 0; i < QPT; ++i) {
            const int q = threadIdx.x + i * NTH;
            const int row = q / QROW, col = (q % QROW) * 4;
            const int m = m0 + row, n = nt0 * 16 + col;
            if (q < NQ && m < g.M) {
                *reinterpret_cast<f32x4 *>(g.out + (size_t)m * g.ldo + n) = dswish4(summed4(row * Cfg::LDR + col) + bq[i]);
            }
        }
    } else {   // EPI_LSTM: each 4-column group = gates i,f,g,o of one hidden unit
        // (layer-major) the input halves of all of this thread's quads, fetched up front: a load inside the loop below makes
        // the compiler wait for ALL outstanding memory operations at the loop's merge points, i.e. for the previous quad's
        // STORES (~0.5 us each, three times per 64x64 tile) -- also on the streaming path, which loads nothing here
        f32x4 pq[QPT];
        if (g.p_add) {
#pragma unroll
            for (int i = 0; i < QPT; ++i) {
                int m = qm[i];
                if (m >= g.M) m = g.M - 1;
                pq[i] = *reinterpret_cast<const f32x4 *>(g.p_add + (size_t)m * g.ldp + qunit[i] * 4);
            }
        }
        // every load this epilogue depends on (previous cell values, biases, input halves) has been issued long ago: settle them
        // here, once, so that nothing in the loop waits on the memory counter while the previous quad's stores are in flight
        __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0) only (expcnt / lgkmcnt fields at their maxima)
#pragma unroll
        for (int i = 0; i < QPT; ++i) {
            // x = y * scale(y) entered the GEMM as y: waves 0 and 1 hold the input half of the sum, which takes the row's scale here
            f32x4 gt;
            if (g.p_add || NEED_SCL) {
                const int o = qo[i];
                const f32x4 p2 = *reinterpret_cast<const f32x4 *>(red + 2 * PLANE + o), p3 = *reinterpret_cast<const f32x4 *>(red + 3 * PLANE + o);
                f32x4 xin;
                if (g.p_add) {           // layer-major: the input half was computed for all time steps at once (EPI_XPART)
                    xin = pq[i];
                } else {
                    const f32x4 p0 = *reinterpret_cast<const f32x4 *>(red + o), p1 = *reinterpret_cast<const f32x4 *>(red + PLANE + o);
                    xin = gate_xin(p0, p1, scl[(threadIdx.x + i * NTH) / QROW]);
                }
                gt = gate_combine(xin, p2, p3, qb[i]);
            } else {
                gt = summed4(qo[i]) + qb[i];
            }
            const LstmCell cell = lstm_cell(gt, cprev[i]);
            const float u = g.debug == 2 ? gt.x + gt.y + gt.z + gt.w : cell.u;      // (measurement only)
            if (qok[i]) { *cptr[i] = cell.c_new; g.out[(size_t)qm[i] * g.ldo + qunit[i]] = u; }
        }
    }
    stamp(4);
}

template <int MT, int NT, int EPI, int AOP, int WT, int MODE, int ASM>
__global__ __launch_bounds__(256, (MT == 4 && !ASM) ? 2 : 1) void gemm_f32_kernel(GemmArgs g)
{
    if constexpr (EPI == EPI_LSTM) stamp_begin(g.stamp);
    gemm_body<MT, NT, EPI, AOP, WT, MODE, ASM>(g, (int)blockIdx.z, blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z), (int)blockIdx.x, (int)blockIdx.y, gridDim.y == 1);
    if constexpr (EPI == EPI_LSTM) stamp_end(g.stamp);
}

// The same GEMM for `gridDim.z / zdiv` INDEPENDENT problems of one shape in one launch: blockIdx.z / zdiv selects the argument
// block (a device array written before the launch, read with scalar loads), blockIdx.z % zdiv is the slab group.  The
// offline wavefront schedule (engine.cc) batches the same step of all encoder layers this way: at one session a layer's
// recurrent step is a latency-bound launch, twelve of them in one launch cost about the same.
template <int MT, int NT, int EPI, int AOP, int WT, int MODE, int ASM>
__global__ __launch_bounds__(256, (MT == 4 && !ASM) ? 2 : 1) void gemm_f32_zkernel(const GemmArgs *__restrict__ zargs, int zdiv)
{
    const int zl = (int)blockIdx.z / zdiv;
    // a plain copy through the read-only, non-aliased kernel argument: uniform address -> scalar loads.  (The pointer members
    // are generic to the compiler -- flat_load / flat_store instead of global_load with an SGPR base -- and neither assumptions
    // nor address-space round trips change that; measured against the by-value kernel at one problem per launch: no difference.)
    const GemmArgs g = zargs[zl];
    if constexpr (EPI == EPI_LSTM) stamp_begin(g.stamp);
    gemm_body<MT, NT, EPI, AOP, WT, MODE, ASM>(g, (int)blockIdx.z - zl * zdiv, blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z), (int)blockIdx.x, (int)blockIdx.y, gridDim.y == 1);
    if constexpr (EPI == EPI_LSTM) stamp_end(g.stamp);
}

// Balanced form of the z-batched launch for tile counts that are not a whole number of rounds (three 256-row gate problems =
// 768 tiles on 512 resident workgroups): `slots` workgroups walk the tile list with that stride, tile id = x + gx (y + gy z),
// so a CU's two resident workgroups get three tiles between them (slot s takes s and s + slots: the same x, i.e. the same
// XCD and weight column stripe, as in the plain launch).  The plain launch leaves the placement of the last 256 workgroups to
// the dispatcher: they land wherever a slot frees first, some CUs take two of them and the launch waits for those (measured
// 58 us or 70 us per launch, at random; profiles/r04e_b256_streams_under_rocprof.txt).  Same body, same arguments per tile.
template <int MT, int NT, int EPI, int AOP, int WT, int MODE, int ASM>
__global__ __launch_bounds__(256, (MT == 4 && !ASM) ? 2 : 1) void gemm_f32_zkernel_walk(const GemmArgs *__restrict__ zargs, int zdiv, int gx, int gy, int ntiles)
{
    // (at most two tiles per workgroup, as two straight-line copies of the body: a loop around it costs 20 registers, which
    // takes the hand-scheduled 64 x 64 tile over 256 and the kernel down to one workgroup per CU)
    unsigned long long *stamp = nullptr;                         // (gates clock: the slot of the launch = of any of its problems)
    {
        const int tile = (int)blockIdx.x;
        const int bx = tile % gx, r = tile / gx, by = r % gy, bz = r / gy;
        const int zl = bz / zdiv;
        const GemmArgs g = zargs[zl];
        if constexpr (EPI == EPI_LSTM) { stamp = g.stamp; stamp_begin(stamp, blockIdx.x == 0); }
        gemm_body<MT, NT, EPI, AOP, WT, MODE, ASM>(g, bz - zl * zdiv, (unsigned)tile, bx, by, gy == 1);
    }
    const int tile = (int)blockIdx.x + (int)gridDim.x;
    if (tile < ntiles) {
        __syncthreads();                                         // the first tile's epilogue is done with the LDS planes
        const int bx = tile % gx, r = tile / gx, by = r % gy, bz = r / gy;
        const int zl = bz / zdiv;
        const GemmArgs g = zargs[zl];
        gemm_body<MT, NT, EPI, AOP, WT, MODE, ASM>(g, bz - zl * zdiv, (unsigned)tile, bx, by, gy == 1);
    }
    if constexpr (EPI == EPI_LSTM) stamp_end(stamp, gridDim.x, blockIdx.x);
}

// Mixed tiles for a z-batched launch whose 64 x 64 tiles are not a whole number of rounds (FFN up, three 256-row problems = 384 tiles: half
// of the CUs get two workgroups, half one, and the launch takes as long as four problems): the first n - 1 problems on 64 x 64 tiles, the
// last one on 64 x 32 -- 256 + 256 workgroups, every CU one of each.  One-dimensional grid, big tiles first (the dispatcher deals the
// first 256 workgroups one per CU).  Same bodies, same arguments per tile: the sums do not depend on the tile shape.
template <int EPI, int AOP, int MODE>
__global__ __launch_bounds__(256, 1) void gemm_f32_zkernel_mixed(const GemmArgs *__restrict__ zargs, int gx4, int gy, int nbig_problems)
{
    const int nbig = gx4 * gy * nbig_problems;
    int tile = (int)blockIdx.x;
    if (tile < nbig) {
        const int bx = tile % gx4, r = tile / gx4, by = r % gy, z = r / gy;
        const GemmArgs g = zargs[z];
        gemm_body<4, 4, EPI, AOP, 0, MODE, 1>(g, 0, (unsigned)tile, bx, by, gy == 1);
    } else {
        tile -= nbig;
        const int gx2 = 2 * gx4, bx = tile % gx2, by = tile / gx2;
        const GemmArgs g = zargs[nbig_problems];
        gemm_body<4, 2, EPI, AOP, 0, MODE, 1>(g, 0, (unsigned)(nbig + tile), bx, by, gy == 1);
    }
}

// ---------------------------------------------------------------- host side
ProfileEvents &tl_profile_events() { static thread_local ProfileEvents pe; return pe; }
void gemm_profile_next_launch(hipEvent_t start, hipEvent_t stop) { ProfileEvents &pe = tl_profile_events(); pe.a = start; pe.b = stop; }
bool gemm_profile_pending() { return tl_profile_events().a != nullptr; }

// The process's knobs (gemm_plan.h): the environment, read once, and the bench tools' pins
static GemmKnobs &knobs()
{
    static GemmKnobs k = [] {
        GemmKnobs e;
        e.fullk = env_int("APRIL_FULLK", 1); e.gm_tile = env_int("APRIL_GM_TILE", 1);
        e.gm_pp = env_int("APRIL_GM_PP", 1); e.pp_mt = env_int("APRIL_PP_MT", 0); e.pp_wide = env_int("APRIL_PP_WIDE", 1);
        e.tile_big = env_int("APRIL_TILE_BIG", 1); e.tile_f16_fullk = env_int("APRIL_TILE_F16_FULLK", 1);
        e.gm_kw = env_int("APRIL_GM_KW", 1); e.kw_mt = env_int("APRIL_KW_MT", 0); e.kw_over_tile = env_int("APRIL_KW_OVER_TILE", 1);
        e.z_tiles = env_int("APRIL_Z_TILES", 2);
        return e;
    }();
    return k;
}
void gemm_tile_pin(int enable, int mt, int zs) { GemmKnobs &k = knobs(); k.tile_enable = enable; k.tile_pin_mt = mt; k.tile_pin_zs = zs; }
void gemm_pp_pin(int enable, int mt) { GemmKnobs &k = knobs(); k.pp_enable = enable; k.pp_pin_mt = mt; }
void gemm_kw_pin(int enable, int mt) { GemmKnobs &k = knobs(); k.kw_enable = enable; k.kw_pin_mt = mt; }

GemmQuery gemm_query(const GemmArgs &g)
{
    GemmQuery q;
    q.M = g.M; q.N = g.N; q.K = g.K; q.K0 = g.K0; q.K1 = g.K1; q.kz = g.kz; q.epi = g.epi; q.a_op = g.a_op; q.wt = g.wt; q.wave_mask = g.wave_mask;
    q.has_p_add = g.p_add != nullptr; q.has_x_scale = g.x_scale.ssq != nullptr;
    q.zcount = g.zcount; q.tile_ok = g.tile_ok; q.force_fullk = g.force_fullk;
    q.recur_form = recur_form(g); q.kw_ok = gemm_kw_waves(g) != 0; q.pp_ok = gemm_pp_ok(g, 16); q.pw_ok = gemm_pw_ok(g);
    return q;
}
GemmPlan gemm_plan(const GemmArgs &g) { return plan_gemm(gemm_query(g), knobs()); }

[[noreturn]] static void plan_die(const GemmArgs &g, int error)
{
    switch (error) {
    case PLAN_ALWAYS_TILE_OPERANDS: fprintf(stderr, "libapril(mi355x): launch_gemm: always-tile GEMM with a prologue / wave mask / odd N\n"); break;
    case PLAN_NO_TILE_PLAN: fprintf(stderr, "libapril(mi355x): launch_gemm: no GM_TILE plan for an always-tile GEMM (M=%d N=%d kz=%d)\n", g.M, g.N, g.kz); break;
    case PLAN_ROW_NEEDS_FULLK: fprintf(stderr, "libapril(mi355x): launch_gemm: row epilogue %d needs the full-K plan (M=%d N=%d kz=%d)\n", g.epi, g.M, g.N, g.kz); break;
    default: fprintf(stderr, "libapril(mi355x): launch_gemm: x_scale needs K0 == K / 2 and kz == 1\n"); break;
    }
    abort();
}

// the plan and the measurement knobs into the argument block
static void finalize_gemm(GemmArgs &g, const GemmPlan &p)
{
    static const int dbg = env_int("APRIL_GEMM_DEBUG", 0);
    static const int asm_loop = env_int("APRIL_GEMM_ASM", 1);     // 0 = compiler-scheduled loop everywhere (A/B)
    if (p.error) plan_die(g, p.error);
    g.zs = p.zs; g.mode = p.mode; g.debug = dbg;
    // hand-scheduled K loop wherever it exists (fused-epilogue 64x64 / 64x32 fp32 tiles).  Round-2 measurements
    // (tools/gemm_bench, gates [M,1024]x[1024,4096] + LSTM cell, us per launch at M = 512 / 1024 / 2048):
    //   hand loop, no skew 42.2 / 85.6 / 159.2   hand loop, skew 2: 85.5 / 174.3   compiler loop, skew 2 (round-1 choice at two
    //   workgroups per CU): 91.3 / 170.4   compiler loop, no skew: 56.5 / 100.7 / 180.2;  FFN-up [2048,512]x[512,2048]: 42.3 vs 45.7
    g.asm_loop = asm_loop != 0;
}

// One K-split kernel: g itself (dev_args == null) or, where the z-batched kernel exists (Z), n problems of g's shape at dev_args
template <int MT, int NT, int EPI, int AOP, int MODE, bool Z>
static void launch_one(const GemmArgs &g, const GemmArgs *dev_args, int n, hipStream_t s)
{
    constexpr bool HAS_ASM = MODE == GM_SLAB && MT == 4 && (NT == 4 || NT == 2) && AOP == AOP_NONE && (EPI == EPI_LSTM || EPI == EPI_BIAS_DSWISH);
    using Cfg = TileCfg<MT, NT>;
    const int zdiv = MODE == GM_FULLK ? 1 : g.kz / g.zs;
    dim3 grid((unsigned)(g.N / Cfg::BN), (unsigned)((g.M + Cfg::BM - 1) / Cfg::BM), (unsigned)(zdiv * (dev_args ? n : 1)));
    const size_t lds = (Cfg::LDS_FLOATS + scale_lds_floats(g, Cfg::BM)) * sizeof(float);
    const bool hand_loop = HAS_ASM && g.asm_loop && g.debug != 1;
    if constexpr (Z) if (dev_args) {
        if (g.wt == 1) { APRIL_LAUNCH((gemm_f32_zkernel<MT, NT, EPI, AOP, 1, MODE, 0>), grid, dim3(256), lds, s, dev_args, zdiv); return; }
        if constexpr (HAS_ASM) if (hand_loop) {
            if constexpr (EPI == EPI_LSTM && MT == 4 && NT == 4) {
                // APRIL_GEMM_WALK (1): 512 walking workgroups when the launch is more than one round of the chip's 512 resident
                // 64 x 64 gate workgroups but not a whole number of rounds
                static const int walk = env_int("APRIL_GEMM_WALK", 1);
                const long ntiles = (long)grid.x * grid.y * grid.z;
                if (walk && ntiles > 512 && ntiles < 1024) {
                    APRIL_LAUNCH((gemm_f32_zkernel_walk<MT, NT, EPI, AOP, 0, MODE, 1>), dim3(512), dim3(256), lds, s, dev_args, zdiv, (int)grid.x, (int)grid.y, (int)ntiles);
                    return;
                }
            }
            if constexpr (EPI == EPI_BIAS_DSWISH && MT == 4 && NT == 4 && MODE == GM_SLAB) {
                // APRIL_FF1_MIXED (round 6): see gemm_f32_zkernel_mixed
                static const int mixed = env_int("APRIL_FF1_MIXED", 1);      // 256 sessions: 1.341 -> 1.320 ms per step (three alternations on one box)
                const long t4 = (long)grid.x * grid.y, total = t4 * n;
                if (mixed && zdiv == 1 && n >= 2 && total % 256 != 0 && ((long)(n - 1) * t4) % 256 == 0 && (2 * t4) % 256 == 0 && g.N % 32 == 0) {
                    APRIL_LAUNCH((gemm_f32_zkernel_mixed<EPI, AOP, MODE>), dim3((unsigned)((n - 1) * t4 + 2 * t4)), dim3(256), lds, s, dev_args, (int)grid.x, (int)grid.y, n - 1);
                    return;
                }
            }
            APRIL_LAUNCH((gemm_f32_zkernel<MT, NT, EPI, AOP, 0, MODE, 1>), grid, dim3(256), lds, s, dev_args, zdiv); return;
        }
        APRIL_LAUNCH((gemm_f32_zkernel<MT, NT, EPI, AOP, 0, MODE, 0>), grid, dim3(256), lds, s, dev_args, zdiv); return;
    }
    if (g.wt == 1) { APRIL_LAUNCH((gemm_f32_kernel<MT, NT, EPI, AOP, 1, MODE, 0>), grid, dim3(256), lds, s, g); return; }
    if constexpr (HAS_ASM) if (hand_loop) { APRIL_LAUNCH((gemm_f32_kernel<MT, NT, EPI, AOP, 0, MODE, 1>), grid, dim3(256), lds, s, g); return; }
    APRIL_LAUNCH((gemm_f32_kernel<MT, NT, EPI, AOP, 0, MODE, 0>), grid, dim3(256), lds, s, g);
}

// (epilogue, prologue, schedule) combinations that exist, and whether the z-batched kernel does (Z); everything else is a programming error
template <int MT, int NT>
static bool dispatch(const GemmArgs &g, const GemmArgs *dev_args, int n, hipStream_t s)
{
#define CASE(E, A, MD, Z) if (g.epi == E && g.a_op == A && g.mode == MD && (Z || !dev_args)) { launch_one<MT, NT, E, A, MD, Z>(g, dev_args, n, s); return true; }
    if constexpr (NT == 2) {        // the full-K schedule uses 16/32/64 x 32 tiles only
        CASE(EPI_PARTIAL, AOP_TANH_ADD, GM_FULLK, false)
        CASE(EPI_HR, AOP_NONE, GM_FULLK, true) CASE(EPI_RESID_SSQ, AOP_NONE, GM_FULLK, true) CASE(EPI_SLOT_STORE, AOP_NONE, GM_FULLK, false)
        CASE(EPI_HR, AOP_NONE, GM_SLAB, true) CASE(EPI_RESID_SSQ, AOP_NONE, GM_SLAB, true) CASE(EPI_SLOT_STORE, AOP_NONE, GM_SLAB, false)
    }
    CASE(EPI_PARTIAL, AOP_NONE, GM_SLAB, false) CASE(EPI_PARTIAL, AOP_TANH_ADD, GM_SLAB, false)
    CASE(EPI_LSTM, AOP_NONE, GM_SLAB, true) CASE(EPI_XPART, AOP_NONE, GM_SLAB, true)
    CASE(EPI_BIAS_DSWISH, AOP_NONE, GM_SLAB, true)
#undef CASE
    return false;
}
// the runtime tile of the K-split kernels (16 mt x 16 nt) as template arguments
template <int MT>
static bool dispatch_nt(int nt, const GemmArgs &g, const GemmArgs *dev_args, int n, hipStream_t s)
{
    return nt == 4 ? dispatch<MT, 4>(g, dev_args, n, s) : nt == 2 ? dispatch<MT, 2>(g, dev_args, n, s) : dispatch<MT, 1>(g, dev_args, n, s);
}

// The one dispatch: g finalized with plan p; dev_args != null: n problems of g's shape in device memory
static void launch_planned(const GemmArgs &g, const GemmPlan &p, const GemmArgs *dev_args, int n, hipStream_t s)
{
    switch (p.route) {
    case ROUTE_STREAM: launch_recur(g, p.form, dev_args, dev_args ? n : 1, s); return;
    case ROUTE_PW: launch_gemm_pw(g, dev_args, n, s); return;
    case ROUTE_PP: launch_gemm_pp(g, p.mt, dev_args, n, s); return;
    case ROUTE_TILE: launch_gemm_tile(g, p.mt, p.nt, dev_args, n, s); return;
    case ROUTE_KW: launch_gemm_kw(g, p.mt, p.nt, dev_args, n, s); return;
    }
    const bool ok = p.mt == 1 ? dispatch_nt<1>(p.nt, g, dev_args, n, s) : p.mt == 2 ? dispatch_nt<2>(p.nt, g, dev_args, n, s) : dispatch_nt<4>(p.nt, g, dev_args, n, s);
    if (!ok) { fprintf(stderr, "libapril(mi355x): %s: no kernel for epi %d a_op %d mode %d tile %dx%d\n", dev_args ? "launch_gemm_z" : "launch_gemm", g.epi, g.a_op, g.mode, p.mt, p.nt); abort(); }
}

// (a launch runs what plan_launch says of exactly this block: the engine's question, gemm_plan, is asked before the block is chosen)
void launch_gemm(const GemmArgs &g_in, hipStream_t s)
{
    GemmArgs g = g_in;
    const GemmPlan p = plan_launch(gemm_query(g), knobs());
    if (p.route != ROUTE_STREAM) finalize_gemm(g, p);      // (the stream kernels read neither the plan nor the knobs)
    launch_planned(g, p, nullptr, 0, s);
}

// ---- n independent problems of one shape in one launch
void stage_gemm_z(const GemmArgs *items, int n, GemmArgs *staged)
{
    GemmPlan p0;
    for (int i = 0; i < n; ++i) {
        staged[i] = items[i];
        staged[i].zcount = n;
        const GemmPlan p = plan_launch(gemm_query(staged[i]), knobs());
        finalize_gemm(staged[i], p);
        if (i == 0) p0 = p;
        const GemmArgs &a = staged[i], &b = staged[0];
        if (p.mt != p0.mt || p.nt != p0.nt || p.zs != p0.zs || p.mode != p0.mode || a.M != b.M || a.N != b.N || a.K != b.K || a.kz != b.kz || a.epi != b.epi || a.wt != b.wt ||
            a.a_op != AOP_NONE || a.x_scale.groups != b.x_scale.groups || a.r_scale.groups != b.r_scale.groups || (a.x_scale.ssq == nullptr) != (b.x_scale.ssq == nullptr)) {
            fprintf(stderr, "libapril(mi355x): stage_gemm_z: the problems of one launch must have one shape\n"); abort();
        }
    }
}

void launch_gemm_z(const GemmArgs *staged, int n, const GemmArgs *dev_args, hipStream_t s)
{
    if (n <= 0) return;
    // (stage_gemm_z checked that the n problems have one shape, and finalized them)
    launch_planned(staged[0], plan_launch(gemm_query(staged[0]), knobs()), dev_args, n, s);
}

// ---- the planner for CPU-side tests (include/aprilx_engine.h): no GPU call
}  // namespace aprilx
using namespace aprilx;

int aprilx_plan_gemm(int M, int N, int kz, int zcount, int tile_ok, int force, int32_t *out)
{
    if (!out || M <= 0 || N <= 0 || kz <= 0 || zcount <= 0) return -1;
    // the question of a row-epilogue GEMM of this shape: fused?  planes of its partial form; would the occupancy rule (tile_ok 1) plan GM_TILE?
    GemmQuery q; q.M = M; q.N = N; q.kz = kz; q.zcount = zcount; q.tile_ok = tile_ok; q.force_fullk = force; q.epi = EPI_HR;
    const GemmPlan part = plan_partial_form(q, knobs());
    if (part.error) return -1;
    out[0] = row_fused(q, knobs()) ? 1 : 0;
    out[1] = part.planes;
    q.tile_ok = 1;
    out[2] = plan_partial_form(q, knobs()).mode == GM_TILE ? 1 : 0;
    return 0;
}
// in: M N K K0 K1 kz epi a_op wt wave_mask p_add? x_scale? zcount tile_ok force_fullk lda0 x_scale.groups r_scale.groups(0: none) out? out16? state16? ssq_out?
// out: the capabilities gemm_query finds (recur_form, kw, pp, pw) and gemm_plan's route form mode mt nt zs planes fused error.  No GPU call.
int aprilx_gemm_plan_debug(const int32_t *in, int32_t *out)
{
    if (!in || !out) return -1;
    static float dummy[4];
    GemmArgs g;                                       // only which pointers are set matters to the capability predicates
    g.M = in[0]; g.N = in[1]; g.K = in[2]; g.K0 = in[3]; g.K1 = in[4]; g.kz = in[5]; g.epi = in[6]; g.a_op = in[7]; g.wt = in[8]; g.wave_mask = in[9];
    if (in[10]) g.p_add = dummy;
    if (in[11]) { g.x_scale.ssq = dummy; g.x_scale.groups = in[16]; }
    g.zcount = in[12]; g.tile_ok = in[13]; g.force_fullk = in[14]; g.lda0 = in[15];
    if (in[17]) { g.r_scale.ssq = dummy; g.r_scale.groups = in[17]; }
    if (in[18]) g.out = dummy;
    if (in[19]) g.out16 = dummy;
    if (in[20]) g.state16 = dummy;
    if (in[21]) g.ssq_out = dummy;
    const GemmQuery q = gemm_query(g);
    const GemmPlan p = gemm_plan(g);
    const int32_t r[13] = {q.recur_form, q.kw_ok, q.pp_ok, q.pw_ok, p.route, p.form, p.mode, p.mt, p.nt, p.zs, p.planes, p.fused, p.error};
    std::copy(r, r + 13, out);
    return 0;
}
