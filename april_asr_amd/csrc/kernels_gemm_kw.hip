// GM_KW schedule of the MFMA GEMM (kernels.h) for gfx950: the waves of a workgroup split K (as GM_FULLK does), but the
// ACTIVATION operand of every wave arrives in full 128-byte lines through a wave-private LDS ring (global_load_lds_dwordx4),
// the weights stay on the direct register stream.
//
// Why it exists (round 5): the N = d_model GEMMs of a layer (LSTM projection K = hidden, FFN down K = ffn) at 256..768 rows per
// launch ran as 16 x 32 full-K tiles whose A fragment load -- lane (i, kq) reads 16 bytes of row i -- touches sixteen cache lines
// per quarter wave, 64 bytes used of each: the CU's vector cache delivered ~24 B/clk and the kernels sat at 0.26 / 0.35 of the
// fp32 MFMA peak (profiles/r04_b256_kernel_stats.csv), twice the MFMA time in operand waits.  GM_TILE (waves split the OUTPUT tile,
// operands shared through LDS) needs 64 x 64 tiles to pay and a 256-row, N = 512 problem has only 32 of those.  Here the tile stays
// small (32 x 32 outputs: 128 workgroups per 256-row problem, one eight-wave workgroup per CU at two problems per launch) and K is
// split across the EIGHT waves; since every wave owns its own k range nothing is shared, so there is no barrier in the K loop --
// each wave runs its own DMA ring: a stage is two k blocks = 128 bytes of each of the tile's rows (8 rows per 1 KB DMA
// instruction, eight full lines), stored with the 16-byte segments of row R xor-swizzled by (R >> 1) & 7 so that the MFMA A
// fragment read (ds_read_b128) is conflict-free (the layout of kernels_gemm_tile.hip).
//
// Canonical summation (kernels.h) is kept exactly: a chunk is one in-order MFMA chain over its k blocks, a slab is
// ((c0 + c1) + c2) + c3, slabs meet pairwise in slab order.  Wave w owns chunks [w cpw, (w + 1) cpw), cpw = 4 kz / NW:
//   cpw >= 4  whole slabs: folded in registers (S, then R = S0 + S1 for two slabs), the waves meet once as the balanced tree
//             ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7))
//   cpw == 1  one chunk per wave: the planes meet as ((p0 + p1) + p2) + p3 per slab, two slabs (kz = 2) as s0 + s1
// => bit-identical to GM_SLAB / GM_FULLK / GM_TILE at any batch size (tools/kw_bench compares every output bitwise; the engine's
// batch-invariance tests cross the schedule boundary).
// Epilogues: EPI_HR (projection), EPI_RESID_SSQ (FFN down), term by term those of gemm_body.
// Replaces the MatMul nodes of the encoder graph (reference call site src/april_session.c:131-148).
#include "kernels.h"
#include "device_utils.h"
#include "env.h"
#include "gemm_kw_asm.inc"
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>

namespace aprilx {

namespace {

template <class T> __device__ __forceinline__ T gload(const void *p) { return *(const __attribute__((address_space(1))) T *)(p); }
template <class T> __device__ __forceinline__ void gstore(void *p, const T &v) { *(__attribute__((address_space(1))) T *)(p) = v; }

template <int N> __device__ __forceinline__ void wait_vm()
{
    // s_waitcnt vmcnt(N) only (gfx9 encoding: vmcnt[3:0] in bits 3:0, vmcnt[5:4] in bits 15:14; expcnt / lgkmcnt at their maxima)
    __builtin_amdgcn_s_waitcnt(0x0F70 | (N & 15) | ((N >> 4) << 14));
}
__device__ __forceinline__ void wait_lgkm0() { __builtin_amdgcn_s_waitcnt(0xC07F); }      // lgkmcnt(0) only

// Tile 16 MT x 16 NT per workgroup, NW waves splitting K, D ring stages per wave (four stages measured the same at twice the LDS: LAB_NOTES.md)
constexpr int NW = 8, D = 2;
template <int MT, int NT> struct KwGeom {
    static constexpr int BM = 16 * MT, BN = 16 * NT, LDR = BN + 4, NTH = 64 * NW;
    static constexpr int STAGE_BYTES = BM * 128;                          // two k blocks of the tile's rows
    static constexpr int RING_BYTES = D * STAGE_BYTES, PLANE_BYTES = BM * LDR * 4;
    static constexpr int WAVE_BYTES = ((RING_BYTES > PLANE_BYTES ? RING_BYTES : PLANE_BYTES) + 1023) / 1024 * 1024;
    static constexpr int LDS_MAIN = NW * WAVE_BYTES;
    static constexpr int PLANE = WAVE_BYTES / 4;                          // floats between the waves' planes
    static constexpr int NPIECE = 2 * MT;                                 // 1 KB DMA pieces per stage
    static constexpr int LX = NPIECE, LY = 2 * NT, GSZ = LX + LY;         // memory operations per stage: {DMA pieces}, {B of k blocks 0, 1}
};

// HAND: the K loop is the hand-placed instruction stream of gemm_kw_asm.inc (tools/gen_kw_asm.py) instead of the compiler-scheduled
// stages below -- same memory operations in the same order, same chains, same fold; APRIL_KW_ASM=0 selects the compiler's loop (A/B)
template <int MT, int NT> constexpr bool kw_has_hand(int cpw) { return NT == 2 && (MT == 1 || MT == 2) && cpw == 4; }

template <int MT, int NT, int EPI, int CPW, bool HAND>
__device__ __forceinline__ void gemm_kw_body(const GemmArgs &g, const int bx, const int by, const unsigned wg_linear)
{
    using G = KwGeom<MT, NT>;
    constexpr int BM = G::BM, BN = G::BN, LDR = G::LDR, NTH = G::NTH, PLANE = G::PLANE;
    constexpr bool ROW_EPI = EPI == EPI_HR || EPI == EPI_RESID_SSQ;
    static_assert(ROW_EPI, "no GM_KW form of this epilogue");
    static_assert(CPW == 1 || CPW == 4, "a wave owns one chunk or one slab");
    static_assert(!HAND || kw_has_hand<MT, NT>(CPW), "no hand-placed loop for this form");
    constexpr bool DB1 = MT * NT >= 16;                    // 64 x 64 wave tiles: the register-lean form of the K loop (below)
    extern __shared__ __attribute__((aligned(1024))) float red[];
    char *lds = reinterpret_cast<char *>(red);

    if (g.run_flag && gload<int>(g.run_flag) != g.run_gen) return;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#ifdef APRIL_KW_ABLATE
    // measurement only (tools/kw_bench_ablate, APRIL_GEMM_DEBUG): 3 .. 9 as at their uses below; 10 / 11 = 6 / 7 without the fold
    // (profiles/kw_loop_ablation.txt: what the loop costs without its global-memory instructions, term by term)
    const bool abl_nofold = g.debug == 10 || g.debug == 11;
    const int abl = g.debug == 10 ? 6 : g.debug == 11 ? 7 : g.debug;
#endif
    // measurement only (tools/kw_bench built with -DAPRIL_GEMM_TRACE): s_memtime stamps of wave 0 at the phase boundaries
#ifdef APRIL_GEMM_TRACE
    auto stamp = [&](int i) { if (g.trace && wave == 0) g.trace[(size_t)wg_linear * 16 + i] = __builtin_amdgcn_s_memtime(); };
    unsigned long long ph_acc[5] = {0, 0, 0, 0, 0}, ph_t = 0;
    auto lap = [&](int i) { const unsigned long long now = __builtin_amdgcn_s_memtime(); ph_acc[i] += now - ph_t; ph_t = now; };
#else
    auto stamp = [](int) {};
    auto lap = [](int) {};
    (void)wg_linear;
#endif
    stamp(0);
    const int nt0 = bx * NT, n0 = bx * BN, m0 = by * BM;
    const int KB = g.K >> 4;
    const int c = KB / (4 * g.kz);                        // k blocks per chunk (even: checked on the host)
    constexpr int cpw = CPW;                              // chunks per wave = 4 kz / NW (checked on the host): one chunk, or one slab
    const int T = cpw * c;                                // k blocks of this wave
    const int first_kb = wave * T;
    const int nstage = T >> 1;                            // a multiple of D, >= D (checked on the host)
    const int cs = c >> 1;                                // stages per chunk

    // ---- BasicNorm scale of the residual rows (EPI_HR): partials fetched first thing, reduced through LDS after the K loop
    const RowScale &rsc = g.r_scale;
    const bool NEED_SCL = EPI == EPI_HR && rsc.ssq != nullptr;
    float *scl = red + G::LDS_MAIN / 4;
    float stg[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    constexpr int TPR = NTH / BM;
    const int ppt = (rsc.groups + TPR - 1) / TPR;
    const bool staged = NEED_SCL && ppt <= 4 && !(MT == 1 || MT * NT >= 16);      // (the register-lean forms fetch the partials behind the loop; NEED_SCL is EPI_HR only)
    const int srow = threadIdx.x / TPR, sj0 = (threadIdx.x % TPR) * ppt;
    if (NEED_SCL && staged) {
        int r = m0 + srow;
        if (r >= g.M) r = g.M - 1;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < ppt && sj0 + k < rsc.groups) stg[k] = gload<float>(rsc.ssq + (size_t)r * rsc.groups + sj0 + k);
    }

    // ---- DMA pieces of this wave: piece i = rows 8 i .. 8 i + 7 of the tile (lane -> row 8 i + (lane >> 3), 16-byte segment
    // lane & 7 of the stage's 128 bytes, swizzled on the SOURCE side: the DMA writes LDS linearly)
    // (uniform 64-bit base that advances with the stage + one 32-bit byte offset per lane and piece: the saddr form of the load;
    // all operands are far below 4 GiB per array)
    uint32_t aoff[G::NPIECE];
    const char *abase = reinterpret_cast<const char *>(g.a0) + (size_t)first_kb * 64;
    {
        const int *aidx = g.aidx0;
        const int lda = g.lda0;
        int arows[G::NPIECE];
#pragma unroll
        for (int i = 0; i < G::NPIECE; ++i) {
            const int row = m0 + i * 8 + (lane >> 3);
            arows[i] = row >= g.M ? g.M - 1 : row;         // padding rows recompute the last row; never stored
        }
        if (aidx) {
#pragma unroll
            for (int i = 0; i < G::NPIECE; ++i) arows[i] = gload<int>(aidx + arows[i]);
        }
#pragma unroll
        for (int i = 0; i < G::NPIECE; ++i) {
            const int R = i * 8 + (lane >> 3);
            const int gseg = (lane & 7) ^ ((R >> 1) & 7);
            aoff[i] = (uint32_t)((size_t)arows[i] * lda * 4 + gseg * 16);
        }
    }
    char *my = lds + wave * G::WAVE_BYTES;
    auto issue_dma = [&](int slot) {
#ifdef APRIL_KW_ABLATE
        if (abl == 4 || abl == 6 || abl == 7 || abl == 9) return;      // measurement: no DMA (stale LDS contents)
#endif
#pragma unroll
        for (int i = 0; i < G::NPIECE; ++i) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(abase + aoff[i]),
                                             (__attribute__((address_space(3))) void *)(my + slot * G::STAGE_BYTES + i * 1024), 16, 0, 0);
        }
#ifdef APRIL_KW_ABLATE
        if (g.debug == 3) return;                          // measurement: every stage re-reads the first one (cache-resident operands)
#endif
        abase += 128;
    };
    // weights: uniform base (advances with the k block) + lane offset; tile nt of k block kb = 1 KB at ((nt0 + nt) KB + kb) 1024
    const char *bp = reinterpret_cast<const char *>(g.wp) + ((size_t)nt0 * KB + first_kb) * 1024;
    const size_t bstride = (size_t)KB * 1024;
    const uint32_t boff = (uint32_t)lane * 16u;
    // 64 x 64 wave tiles keep ONE stage of weights in registers (a k block is 64 MFMAs = 2 k cycles: the next block's weights, issued behind
    // the block that frees their registers, have landed by then); smaller tiles a ring of D stages
    constexpr int DB = DB1 ? 1 : D;
    f32x4 be[DB][NT], bo[DB][NT];
#ifdef APRIL_KW_ABLATE
#pragma unroll
    for (int t = 0; t < DB; ++t)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) { be[t][nt] = f32x4{1.f, 1.f, 1.f, 1.f}; bo[t][nt] = be[t][nt]; }
#endif
    auto load_b = [&](f32x4 (&b)[NT]) {
#ifdef APRIL_KW_ABLATE
        if (abl == 6 || abl == 7 || abl == 8) {      // measurement: no weight loads (the registers stay defined for the compiler)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) asm volatile("" : "+v"(b[nt]));
            return;
        }
#endif
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) b[nt] = gload<f32x4>(bp + nt * bstride + boff);
#ifdef APRIL_KW_ABLATE
        if (g.debug == 3) return;
#endif
        bp += 1024;
    };

    // ---- what the epilogue reads besides the sums: fetched before the K loop (as in gemm_body); the 64 x 64 wave tiles have no registers
    // to park it in during the loop (accumulators + slab sums + a stage of weights = 224 of 256) and fetch it behind the loop instead
    constexpr int QROW = BN / 4, NQ = BM * QROW, QPT = (NQ + NTH - 1) / NTH;
    f32x4 e_bias[QPT], e_res[QPT];
    int e_slot[QPT];
    bool e_ok[QPT];
    auto fetch_epilogue_operands = [&]() {
#pragma unroll
    for (int i = 0; i < QPT; ++i) {
        const int q = threadIdx.x + i * NTH;
        int m = m0 + q / QROW;
        e_ok[i] = q < NQ && m < g.M;
        if (m >= g.M) m = g.M - 1;
        const int qn = q < NQ ? n0 + (q % QROW) * 4 : n0;
        e_bias[i] = (EPI != EPI_HR) ? gload<f32x4>(g.bias + qn) : f32x4{0.f, 0.f, 0.f, 0.f};
        e_slot[i] = (EPI == EPI_HR && g.slot_idx) ? gload<int>(g.slot_idx + m) : m;
        e_res[i] = (EPI == EPI_HR || (EPI == EPI_RESID_SSQ && g.resid)) ? gload<f32x4>(g.resid + (size_t)m * g.ldr + qn) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    };
    // (16-row projection tiles: 80 registers = six waves per SIMD = three workgroups per CU, so that the 768 workgroups of a three-problem
    // launch are ONE round: 17.7 -> 14.7 us; FFN down, twice the K, is operand-issue bound and LOSES with the third workgroup: 22.5 -> 24.5 us)
    constexpr bool LATE_EPI = DB1 || (MT == 1 && EPI == EPI_HR);
    if constexpr (!LATE_EPI) fetch_epilogue_operands();

    // ---- fragment addresses inside a stage buffer: k block p, m tile mt: row 16 mt + mrow, segment (4 p + kq) ^ ((mrow >> 1) & 7)
    const int mrow = lane & 15, kq = lane >> 4;
    int a_rd[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) a_rd[p] = mrow * 128 + (((p * 4 + kq) ^ ((mrow >> 1) & 7)) << 4);
    auto read_frags = [&](int slot, int p, f32x4 (&a)[MT]) {
#ifdef APRIL_KW_ABLATE
        if (abl == 6) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) asm volatile("" : "+v"(a[mt]));
            return;
        }
#endif
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) a[mt] = *reinterpret_cast<const f32x4 *>(my + slot * G::STAGE_BYTES + a_rd[p] + mt * 2048);
    };

    f32x4 acc[MT][NT], S[CPW == 4 ? MT : 1][CPW == 4 ? NT : 1];
#define APRIL_KW_EACH(expr) _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) { expr; }
    APRIL_KW_EACH(acc[mt][nt] = (f32x4{0.f, 0.f, 0.f, 0.f}))
    int chunk_i = 0, in_chunk = 0;
    auto fold = [&]() {                                   // a chunk chain is complete (CPW == 4: S = ((c0 + c1) + c2) + c3)
#ifdef APRIL_KW_ABLATE
        if (abl_nofold) return;
#endif
        if constexpr (CPW == 4) {
            // one accumulator tile at a time (pinned): left alone, the scheduler computes all sums into fresh registers first, which at 64 x 64
            // per wave (64 + 64 registers) overflows the file
            const bool first = chunk_i == 0;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    S[mt][nt] = first ? acc[mt][nt] : S[mt][nt] + acc[mt][nt];
                    acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if constexpr (MT * NT >= 16) __builtin_amdgcn_sched_barrier(0);
                }
            ++chunk_i;
        }
    };
    // k step outermost: consecutive MFMAs go to different accumulators; per accumulator the k steps of a block in order j = 0..3
    // (the canonical chain)
    auto mfma_block = [&](const f32x4 (&a)[MT], const f32x4 (&b)[NT]) {
#ifdef APRIL_KW_ABLATE
        if (g.debug == 5 || g.debug == 8 || g.debug == 9) {      // measurement: no MFMAs (DMA + loads + LDS reads alone); the operands stay live
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) asm volatile("" :: "v"(a[mt]));
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) asm volatile("" :: "v"(b[nt]));
            return;
        }
#endif
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt][j], b[nt][j], acc[mt][nt], 0, 0, 0);
    };

    // ---- K loop.  Stage t = k blocks (2 t, 2 t + 1) of the wave's range: A in ring buffer t % D, B in be / bo [t % D].  Memory
    // operations are issued in the order LX(0) LY(0) .. LX(D-1) LY(D-1) | LX(D) .. LY(D) | ..., LX(t) = {DMA(t)}, LY(t) = {B even(t),
    // B odd(t)}; iteration s issues LX(s + D) behind its first k block (the buffer of stage s has been read: lgkmcnt(0)) and
    // LY(s + D) behind its second, and waits for LX(s + 1) in between -- (D - 1) GSZ younger operations stay in flight (the tail
    // counts down; the weights are register loads, which the compiler's own counts cover).  Nothing here is shared between waves:
    // no barrier.  The stage is [MFMA block][issue][MFMA block][issue] with the two issue halves about equal (FFN down, two problems:
    // 17.0 -> 16.1 us against all issue behind the first block).
    f32x4 a0[MT], a1[MT];
#ifdef APRIL_KW_ABLATE
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) { a0[mt] = f32x4{1.f, 1.f, 1.f, 1.f}; a1[mt] = a0[mt]; }
#endif
    if constexpr (DB1) {
        // one stage of weights in registers, two stages of activation rows in the ring (D == 2).  Issue order: DMA(0) DMA(1) Be(0) Bo(0) |
        // iteration s: {DMA(s + 2), Be(s + 1)} behind the first k block, {Bo(s + 1)} behind the second; the explicit wait in between is for
        // DMA(s + 1), younger than it: Be(s), Bo(s), DMA(s + 2), Be(s + 1) (the weights are register loads: the compiler's own counts)
        if (g.debug != 1) {
            issue_dma(0); issue_dma(1); load_b(be[0]); load_b(bo[0]);
            wait_vm<G::NPIECE + 2 * NT>();                 // DMA(0) has landed
            __builtin_amdgcn_sched_barrier(0);
            read_frags(0, 0, a0);
            stamp(1);
            // m tile outermost: a block's fragment of m tile mt is dead after that tile's 16 MFMAs (k steps in order per accumulator, four
            // accumulators in rotation), so the NEXT block's fragment is read into the same registers right behind them: one fragment set
            auto mfma_mt = [&](int mt, const f32x4 (&b)[NT]) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[mt][j], b[nt][j], acc[mt][nt], 0, 0, 0);
            };
            auto read_frag1 = [&](int slot, int p, int mt) { a0[mt] = *reinterpret_cast<const f32x4 *>(my + slot * G::STAGE_BYTES + a_rd[p] + mt * 2048); };
            for (int s = 0; s < nstage; ++s) {
                const int slot = s & 1;
                const bool more_a = s + 2 < nstage, more_b = s + 1 < nstage;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    mfma_mt(mt, be[0]);
                    __builtin_amdgcn_sched_barrier(0);
                    read_frag1(slot, 1, mt);
                    __builtin_amdgcn_sched_barrier(0);
                }
                wait_lgkm0();                              // both k blocks of the buffer are in registers
                if (more_a) issue_dma(slot);
                if (more_b) load_b(be[0]);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    mfma_mt(mt, bo[0]);
                    __builtin_amdgcn_sched_barrier(0);
                    if (mt == 0) { if (more_a) wait_vm<G::NPIECE + 3 * NT>(); else if (more_b) wait_vm<3 * NT>(); }      // DMA(s + 1) has landed
                    read_frag1(slot ^ 1, 0, mt);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (more_b) load_b(bo[0]);
                if constexpr (CPW == 4) { if (++in_chunk == cs) { in_chunk = 0; fold(); } }
            }
        }
    } else if constexpr (HAND) {
        // the whole loop, its priming loads and the folds in one statement: S comes back in the fixed registers of the generator's plan.
        // Operands: the lanes' byte offsets (DMA pieces, weights, fragment reads with the wave's LDS base added), the wave's uniform bases
        if (g.debug != 1) {
            stamp(1);
            const uint32_t lds_my = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) char *)my);
            const uint32_t rd0 = lds_my + (uint32_t)a_rd[0], rd1 = lds_my + (uint32_t)a_rd[1];
            const char *bp1 = bp + bstride;
            if constexpr (MT == 2) {
                asm volatile(APRIL_KWLOOP_M2_TEXT
                             : APRIL_KWLOOP_M2_S0(S[0][0]), APRIL_KWLOOP_M2_S1(S[0][1]), APRIL_KWLOOP_M2_S2(S[1][0]), APRIL_KWLOOP_M2_S3(S[1][1])
                             : [ao0] "v"(aoff[0]), [ao1] "v"(aoff[1]), [ao2] "v"(aoff[2]), [ao3] "v"(aoff[3]), [bo] "v"(boff), [rd0] "v"(rd0), [rd1] "v"(rd1),
                               [ap] "s"(abase), [bp0] "s"(bp), [bp1] "s"(bp1), [lds] "s"(lds_my), [nst] "s"(nstage), [cs] "s"(cs)
                             : APRIL_KWLOOP_M2_CLOBBERS);
            } else {
                asm volatile(APRIL_KWLOOP_M1_TEXT
                             : APRIL_KWLOOP_M1_S0(S[0][0]), APRIL_KWLOOP_M1_S1(S[0][1])
                             : [ao0] "v"(aoff[0]), [ao1] "v"(aoff[1]), [bo] "v"(boff), [rd0] "v"(rd0), [rd1] "v"(rd1),
                               [ap] "s"(abase), [bp0] "s"(bp), [bp1] "s"(bp1), [lds] "s"(lds_my), [nst] "s"(nstage), [cs] "s"(cs)
                             : APRIL_KWLOOP_M1_CLOBBERS);
            }
        }
    } else
    if (g.debug != 1) {
#pragma unroll
        for (int t = 0; t < D; ++t) { issue_dma(t); load_b(be[t]); load_b(bo[t]); }
        wait_vm<(D - 1) * G::GSZ + G::LY>();               // LX(0) has landed
        __builtin_amdgcn_sched_barrier(0);
        read_frags(0, 0, a0);
        stamp(1);
        auto stage = [&](const int slot, const bool more, auto wait_next) {
            read_frags(slot, 1, a1);
            __builtin_amdgcn_sched_barrier(0);
            mfma_block(a0, be[slot]);
            __builtin_amdgcn_sched_barrier(0);
            lap(0);
            wait_lgkm0();                                  // both k blocks of the buffer are in registers
            lap(1);
            if (more) issue_dma(slot);
            lap(2);
            wait_next();                                   // LX(s + 1) has landed
            lap(3);
            __builtin_amdgcn_sched_barrier(0);
            read_frags(slot + 1 == D ? 0 : slot + 1, 0, a0);
            __builtin_amdgcn_sched_barrier(0);
            mfma_block(a1, bo[slot]);
            __builtin_amdgcn_sched_barrier(0);
            if (more) { load_b(be[slot]); load_b(bo[slot]); }
            if constexpr (CPW == 4) { if (++in_chunk == cs) { in_chunk = 0; fold(); } }
            lap(4);
        };
#ifdef APRIL_GEMM_TRACE
        ph_t = __builtin_amdgcn_s_memtime();
#endif
        int s = 0;
        for (; s + D < nstage; s += D) {
#pragma unroll
            for (int j = 0; j < D; ++j) stage(j, true, [] { wait_vm<(D - 1) * G::GSZ>(); });
        }
        // tail: stages nstage - D .. nstage - 1 (slots 0 .. D - 1), nothing left to issue; younger than LX(s + 1): LY(s + 1) and the
        // whole groups of stages s + 2 .. nstage - 1
        static_assert(D == 2, "the tail below is that of a two-stage ring");
        stage(0, false, [] { wait_vm<G::LY>(); });
        stage(1, false, [] {});
    }
    if constexpr (LATE_EPI) fetch_epilogue_operands();
    stamp(2);
#ifdef APRIL_GEMM_TRACE
    if (g.trace && lane == 0 && (wave == 0 || wave == 4)) {      // phase sums of wave 0 and of wave 4 (the younger wave of the same SIMD, as a rule)
        for (int i = 0; i < 5; ++i) g.trace[(size_t)wg_linear * 16 + (wave == 0 ? 6 : 11) + i] = ph_acc[i];
    }
    if (g.trace && lane == 0) {                            // when the LAST wave of the workgroup left its K loop
        atomicMax(&g.trace[(size_t)wg_linear * 16 + 5], (unsigned long long)__builtin_amdgcn_s_memtime());
    }
#endif

    // ---- the waves meet: every wave parks its result in its own region (its ring is drained: no DMA in flight, all reads done)
    {
        float *mine = red + (size_t)wave * PLANE;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if constexpr (CPW == 4) mine[(mt * 16 + kq * 4 + r) * LDR + nt * 16 + mrow] = S[mt][nt][r];
                    else mine[(mt * 16 + kq * 4 + r) * LDR + nt * 16 + mrow] = acc[mt][nt][r];
                }
    }
    if (NEED_SCL) {
        // the rows' scales: partials (in registers since the first instruction of the kernel, or fetched now) -> LDS, behind the barrier
        // of the meet BM threads add them in column order (rows_scale_park / rows_scale_sum, epilogue.h)
        rows_scale_park<BM, NTH>(scl + BM, rsc, staged, stg, ppt, srow, sj0, m0, g.M, [](const float *p) { return gload<float>(p); });
    }
    __syncthreads();
    if (NEED_SCL) {
        if (threadIdx.x < BM) scl[threadIdx.x] = rows_scale_sum(scl + BM + threadIdx.x * (rsc.groups + 1), rsc);
        __syncthreads();
    }
    stamp(3);
    auto summed4 = [&](int o) {
        const f32x4 p0 = *reinterpret_cast<const f32x4 *>(red + o), p1 = *reinterpret_cast<const f32x4 *>(red + PLANE + o);
        const f32x4 p2 = *reinterpret_cast<const f32x4 *>(red + 2 * PLANE + o), p3 = *reinterpret_cast<const f32x4 *>(red + 3 * PLANE + o);
        const f32x4 p4 = *reinterpret_cast<const f32x4 *>(red + 4 * PLANE + o), p5 = *reinterpret_cast<const f32x4 *>(red + 5 * PLANE + o);
        const f32x4 p6 = *reinterpret_cast<const f32x4 *>(red + 6 * PLANE + o), p7 = *reinterpret_cast<const f32x4 *>(red + 7 * PLANE + o);
        if (cpw >= 4) return ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7));        // eight tree nodes
        return (((p0 + p1) + p2) + p3) + (((p4 + p5) + p6) + p7);                      // two slabs of four chunks
    };
#pragma unroll
    for (int i = 0; i < QPT; ++i) {
        const int q = threadIdx.x + i * NTH;
        const int row = q / QROW, col = (q % QROW) * 4;
        const int m = m0 + row, n = n0 + col;
        const f32x4 v = q < NQ ? summed4(row * LDR + col) : f32x4{0.f, 0.f, 0.f, 0.f};
        if (EPI == EPI_HR) {
            if (e_ok[i]) {
                const HrTail t = hr_tail(v, e_res[i], scl[row]);
                gstore<f32x4>(g.state + (size_t)e_slot[i] * g.ld_state + n, t.state);
                gstore<f32x4>(g.out + (size_t)m * g.ldo + n, t.out);
            }
        } else {   // EPI_RESID_SSQ
            const bool ok = e_ok[i];
            f32x4 y = f32x4{0.f, 0.f, 0.f, 0.f};
            if (ok) {
                y = resid_tail(v, e_bias[i], e_res[i], g.resid != nullptr);
                gstore<f32x4>(g.out + (size_t)m * g.ldo + n, y);
            }
            float ss;                                      // (all lanes take part in the shuffles)
            if (granule_ssq_store(y, ok, q, ss)) gstore<float>(g.ssq_out + (size_t)m * (g.N / SSQ_COLS) + n / SSQ_COLS, ss);
        }
    }
    stamp(4);
#undef APRIL_KW_EACH
}

template <int MT, int NT, int EPI, int CPW, bool HAND>
__global__ __launch_bounds__(64 * NW, (MT == 1 && EPI == EPI_HR) ? 6 : 2) void gemm_kw_kernel(GemmArgs g)
{
    gemm_kw_body<MT, NT, EPI, CPW, HAND>(g, (int)blockIdx.x, (int)blockIdx.y, blockIdx.x + gridDim.x * blockIdx.y);
}

// n independent same-shape problems in one launch (see gemm_f32_zkernel): blockIdx.z picks the argument block
template <int MT, int NT, int EPI, int CPW, bool HAND>
__global__ __launch_bounds__(64 * NW, (MT == 1 && EPI == EPI_HR) ? 6 : 2) void gemm_kw_zkernel(const GemmArgs *__restrict__ zargs)
{
    const GemmArgs g = zargs[blockIdx.z];
    gemm_kw_body<MT, NT, EPI, CPW, HAND>(g, (int)blockIdx.x, (int)blockIdx.y, blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z));
}

template <int MT, int NT, int EPI, int CPW>
void launch_kw_one(const GemmArgs &g, const GemmArgs *dev_args, int n, hipStream_t s)
{
    using G = KwGeom<MT, NT>;
    static const int hand = env_int("APRIL_KW_ASM", 1);      // 0 = the compiler-scheduled K loop everywhere (A/B)
    dim3 grid((unsigned)(g.N / G::BN), (unsigned)((g.M + G::BM - 1) / G::BM), (unsigned)std::max(1, n));
    const size_t lds = (size_t)G::LDS_MAIN + scale_lds_floats(g, G::BM) * sizeof(float);
    if constexpr (kw_has_hand<MT, NT>(CPW)) if (hand && g.debug == 0) {
        launch_gemm_pair<&gemm_kw_kernel<MT, NT, EPI, CPW, true>, &gemm_kw_zkernel<MT, NT, EPI, CPW, true>>(grid, dim3(G::NTH), lds, true, s, g, dev_args);
        return;
    }
    launch_gemm_pair<&gemm_kw_kernel<MT, NT, EPI, CPW, false>, &gemm_kw_zkernel<MT, NT, EPI, CPW, false>>(grid, dim3(G::NTH), lds, true, s, g, dev_args);
}

// (every GEMM gemm_kw_waves accepts has one of these: EPI_HR / EPI_RESID_SSQ, kz 8 / 2 = 4 / 1 chunks per wave)
template <int MT, int NT>
bool dispatch_kw(const GemmArgs &g, const GemmArgs *dev_args, int n, hipStream_t s)
{
    const int cpw = 4 * g.kz / NW;
    if (g.epi == EPI_HR && cpw == 4) { launch_kw_one<MT, NT, EPI_HR, 4>(g, dev_args, n, s); return true; }
    if (g.epi == EPI_HR && cpw == 1) { launch_kw_one<MT, NT, EPI_HR, 1>(g, dev_args, n, s); return true; }
    if (g.epi == EPI_RESID_SSQ && cpw == 4) { launch_kw_one<MT, NT, EPI_RESID_SSQ, 4>(g, dev_args, n, s); return true; }
    if (g.epi == EPI_RESID_SSQ && cpw == 1) { launch_kw_one<MT, NT, EPI_RESID_SSQ, 1>(g, dev_args, n, s); return true; }
    return false;
}

}  // namespace

// GM_KW eligibility of a GEMM (shape + operands): the host-side rule launch_gemm's planner and the engine share.  Returns the
// number of waves (8), or 0.
int gemm_kw_waves(const GemmArgs &g)
{
    if (g.wt != 0 || g.a_op != AOP_NONE || g.wave_mask != 0xF || g.p_add || g.N % 32 != 0 || g.K % 64 != 0) return 0;
    if (g.K1 != 0) return 0;
    if (g.epi != EPI_HR && g.epi != EPI_RESID_SSQ) return 0;
    const int KB = g.K / 16;
    if (KB % (4 * g.kz) != 0) return 0;
    const int c = KB / (4 * g.kz);
    if (c % 2 != 0) return 0;                              // chunks of whole stages
    if (g.kz != 8 && g.kz != 2) return 0;                  // one slab / one chunk per wave
    const int nstage = (4 * g.kz / NW) * c / 2;
    if (nstage < 2 || nstage % 2 != 0) return 0;           // whole rounds of the two-stage ring (the 64 x 64 form takes any nstage >= 2)
    return NW;
}

// launch of a GEMM whose plan chose GM_KW: tile 16 mt x 16 nt, g.zs == g.kz.  The tiles are APRIL_KW_TILES (gemm_plan.h): the planner
// asks the same list before it commits to the schedule, so pinned tile shapes and environment knobs never pick a form that was not
// instantiated
void launch_gemm_kw(const GemmArgs &g, int mt, int nt, const GemmArgs *dev_args, int n, hipStream_t s)
{
    if (gemm_kw_waves(g)) {
#define X(a, b) if (mt == a && nt == b && dispatch_kw<a, b>(g, dev_args, n, s)) return;
        APRIL_KW_TILES(X)
#undef X
    }
    fprintf(stderr, "libapril(mi355x): launch_gemm_kw: no kernel for epi %d tile %d x %d, %d waves\n", g.epi, 16 * mt, 16 * nt, gemm_kw_waves(g));
    abort();
}

}  // namespace aprilx
