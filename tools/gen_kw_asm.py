#!/usr/bin/env python3
"""Generates april_asr_amd/csrc/gemm_kw_asm.inc: the hand-placed K loop of the GM_KW schedule (csrc/kernels_gemm_kw.hip) for its
32 x 32 and 16 x 32 tiles with one slab per wave (CPW == 4): the LSTM projection and the FFN-down GEMM.

What the loop is (the method of tools/gen_gemm_asm.py): one inline-asm statement holds the wave's whole K loop; a stage is two k blocks
= 2 * 4 * MT * NT v_mfma_f32_16x16x4_f32, and every other instruction of the stage is a filler at a fixed place in that stream:

  stage s, slot = s % 2        block 0 = a0 x be[slot]              block 1 = a1 x bo[slot]
  before MFMA 0                vmcnt: be(s) has landed; chunk boundary?  (scalar counter, one branch)
  MFMA 0 .. T-1                chunk boundary: S[t] += acc[t] right in front of tile t's first MFMA of the new chunk, which takes the
                               inline constant 0 as C (the zeroing costs nothing); else the plain MFMAs
  behind MFMA T ..             ds_read_b128 a1 (k block 1 of this slot)
  behind MFMA T+MT+1|2         lgkmcnt(0): the slot has been read -> the 2 MT DMA pieces of stage s + 2, one per gap (M0 written one
                               MFMA ahead of the piece that reads it), activation base += 128
  behind MFMA B-1, B           vmcnt: DMA(s + 1) and bo(s) have landed; ds_read_b128 a0 of stage s + 1 (a block ahead of its use)
  behind MFMA B+2, B+4         be(s + 2): its registers are free since block 0
  behind the last j = 3 MFMA   bo(s + 2) of each n tile, weight bases += 2048, lgkmcnt(0) for a0, loop bookkeeping

Order of memory operations: LX(0) LY(0) LX(1) LY(1) | stage s issues LX(s + 2) LY(s + 2), LX = the DMA pieces, LY = {be nt 0, be nt 1,
bo nt 0, bo nt 1}.  The vmcnt counts are not written by hand: `resolve` replays the stream for several loop lengths, counts the
operations younger than the one a wait needs, and requires every replay of one wait to agree.

Summation: per accumulator the k steps j = 0..3 of a block in order and block after block (the canonical chain); the four (two) tiles
rotate, so dependent MFMAs are T = MT * NT issues apart.  S starts as -0.0 (the identity of the addition, unlike +0.0), so
S = ((c0 + c1) + c2) + c3 is the same sequence of additions as the C++ loop's S = c0; S += c1; ...

Hazards inside the string are the author's: S[t] += acc[t] follows tile t's last MFMA by three other MFMAs (32 x 32: each holds the
matrix pipe for 32 cycles, the result is 40 cycles away) or by one MFMA and an s_nop 7 (16 x 32); M0 is written one instruction ahead
of the DMA that reads it; the final fold waits 16 states.

Register plan: fixed VGPRs from v{BASE} (S, accumulators, two fragment sets, the two-stage weight ring), scalars s80..s90; the S quads
are the statement's outputs (physical-register constraints), everything else a clobber.

usage: gen_kw_asm.py > april_asr_amd/csrc/gemm_kw_asm.inc
"""
NT = 2
BASES = {2: 40, 1: 24}


class Form:
    def __init__(self, MT):
        self.MT, self.T = MT, MT * NT
        self.B = 4 * self.T                    # MFMAs per k block
        self.N = 2 * self.B                    # ... per stage
        self.NPIECE = 2 * MT
        self.STAGE = MT * 16 * 128
        r = BASES[MT]
        self.S = [r + 4 * t for t in range(self.T)]; r += 4 * self.T
        self.ACC = [r + 4 * t for t in range(self.T)]; r += 4 * self.T
        self.A = [[r + 4 * (p * MT + mt) for mt in range(MT)] for p in range(2)]; r += 8 * MT
        self.BQ = [[[r + 4 * ((sl * 2 + p) * NT + nt) for nt in range(NT)] for p in range(2)] for sl in range(2)]; r += 16 * NT
        self.END = r


def quad(r):
    return "v[%d:%d]" % (r, r + 3)


def I(text):
    return ("i", text)


def dma(f, slot, i, rel):
    return ("v", "global_load_lds_dwordx4 %%[ao%d], s[80:81]" % i, ("LX", rel))


def set_m0(f, slot, i):
    return I("s_add_u32 m0, s89, %d" % (slot * f.STAGE + i * 1024))


def load_b(f, slot, p, nt, rel):
    return ("v", "global_load_dwordx4 %s, %%[bo], s[%d:%d]%s" % (quad(f.BQ[slot][p][nt]), 82 + 2 * nt, 83 + 2 * nt, " offset:1024" if p else ""),
            ("bo" if p else "be", rel))


BUMP_A = [I("s_add_u32 s80, s80, 128"), I("s_addc_u32 s81, s81, 0")]
BUMP_B = [I("s_add_u32 s82, s82, 2048"), I("s_addc_u32 s83, s83, 0"), I("s_add_u32 s84, s84, 2048"), I("s_addc_u32 s85, s85, 0")]


def read_a(f, slot, p, mt):
    return I("ds_read_b128 %s, %%[rd%d] offset:%d" % (quad(f.A[p][mt]), p, slot * f.STAGE + mt * 2048))


def mfma(f, slot, p, j, mt, nt, zero_c=False):
    t = mt * NT + nt
    return I("v_mfma_f32_16x16x4_f32 %s, v%d, v%d, %s" % (quad(f.ACC[t]), f.A[p][mt] + j, f.BQ[slot][p][nt] + j, "0" if zero_c else quad(f.ACC[t])))


def fold_tile(f, t):
    return [I("v_add_f32 v%d, v%d, v%d" % (f.S[t] + r, f.S[t] + r, f.ACC[t] + r)) for r in range(4)]


def prime(f):
    out = [I("s_mov_b32 s90, m0"), I("s_mov_b64 s[80:81], %[ap]"), I("s_mov_b64 s[82:83], %[bp0]"), I("s_mov_b64 s[84:85], %[bp1]"),
           I("s_mov_b32 s89, %[lds]"), I("s_lshr_b32 s86, %[nst], 1"), I("s_sub_u32 s86, s86, 1"), I("s_mov_b32 s88, %[cs]"), I("s_mov_b32 s87, 0"),
           I("s_nop 4")]
    for t in range(2):
        for i in range(f.NPIECE):
            out += [set_m0(f, t, i), I("s_nop 0"), dma(f, t, i, t)]
        out += BUMP_A
        out += [load_b(f, t, p, nt, t) for p in range(2) for nt in range(NT)]
        out += BUMP_B
    for t in range(f.T):
        out += [I("v_bfrev_b32 v%d, 1" % (q + r)) for q in (f.S[t], f.ACC[t]) for r in range(4)]      # -0.0
    out.append(("w", [("LX", 0)]))
    out += [read_a(f, 0, 0, mt) for mt in range(f.MT)]
    out.append(I("s_waitcnt lgkmcnt(0)"))
    return out


def stage(f, slot, kind, uid):
    """kind: body (issues stage s + 2), tail0 (stage nstage - 2), tail1 (the last stage)"""
    MT, T, B, N = f.MT, f.T, f.B, f.N
    more, last = kind == "body", kind == "tail1"
    m = [mfma(f, slot, p, j, mt, nt) for p in range(2) for j in range(4) for mt in range(MT) for nt in range(NT)]
    gaps = [[] for _ in range(N)]
    out = [("w", [("be", 0)]), I("s_cmp_eq_u32 s87, 0"), I("s_cbranch_scc0 L_nf%s_%%=" % uid)]
    if MT == 1:
        out.append(I("s_nop 7"))
    for t in range(T):
        out += fold_tile(f, t)
        out.append(mfma(f, slot, 0, 0, t // NT, t % NT, zero_c=True))
    out += [I("s_mov_b32 s87, s88"), I("s_branch L_j%s_%%=" % uid), I("L_nf%s_%%=:" % uid)]
    out += m[:T]
    out.append(I("L_j%s_%%=:" % uid))
    gaps[T].append(I("s_sub_u32 s87, s87, 1"))
    for mt in range(MT):
        gaps[T + mt].append(read_a(f, slot, 1, mt))
    gl = T + MT + (2 if MT == 2 else 1)
    gaps[gl].append(I("s_waitcnt lgkmcnt(0)"))
    if more:
        gaps[gl].append(set_m0(f, slot, 0))
        for i in range(f.NPIECE):
            gaps[gl + 1 + i].append(dma(f, slot, i, 2))
            if i + 1 < f.NPIECE:
                gaps[gl + 1 + i].append(set_m0(f, slot, i + 1))
        gaps[gl + f.NPIECE] += BUMP_A
        assert gl + f.NPIECE <= B - 2
    gaps[B - 1].append(("w", [("bo", 0)] + ([] if last else [("LX", 1)])))
    if not last:
        for mt in range(MT):
            gaps[B - 1 + mt].append(read_a(f, slot ^ 1, 0, mt))
    if more:
        for nt in range(NT):
            gaps[B + 2 + 2 * nt].append(load_b(f, slot, 0, nt, 2))
            gaps[N - T + (MT - 1) * NT + nt].append(load_b(f, slot, 1, nt, 2))
        gaps[N - 1] += BUMP_B
    if not last:
        gaps[N - 1].append(I("s_waitcnt lgkmcnt(0)"))
    if more and slot == 1:
        gaps[N - 1] += [I("s_sub_u32 s86, s86, 1"), I("s_cmp_lg_u32 s86, 0")]
    for g in range(T, N):
        out.append(m[g])
        out += gaps[g]
    assert not any(gaps[:T])
    return out


def resolve(f, blocks):
    """vmcnt(N) of every wait: replay prime + stages for several loop lengths, N = operations issued behind the youngest one needed"""
    counts = {}
    for nstage in (2, 4, 6, 8):
        issued = []                                  # tags in issue order
        seq = [("prime", 0)] + [("body%d" % (s & 1) if s < nstage - 2 else "tail%d" % (s & 1), s) for s in range(nstage)]
        for bname, s in seq:
            for k, it in enumerate(blocks[bname]):
                if it[0] == "v":
                    issued.append((it[2][0], it[2][1] + s))
                elif it[0] == "w":
                    need = [(kind, rel + s) for kind, rel in it[1]]
                    lastpos = max(max(i for i, tg in enumerate(issued) if tg == nd) for nd in need)
                    counts.setdefault((bname, k), set()).add(len(issued) - 1 - lastpos)
    for key, c in counts.items():
        assert len(c) == 1, (key, c)
    return {key: c.pop() for key, c in counts.items()}


def emit(MT, name):
    f = Form(MT)
    blocks = {"prime": prime(f), "body0": stage(f, 0, "body", "b0"), "body1": stage(f, 1, "body", "b1"),
              "tail0": stage(f, 0, "tail0", "t0"), "tail1": stage(f, 1, "tail1", "t1")}
    counts = resolve(f, blocks)
    def text(bname):
        return [it[1] if it[0] != "w" else "s_waitcnt vmcnt(%d)" % counts[(bname, k)] for k, it in enumerate(blocks[bname])]
    out = text("prime")
    out += ["s_cmp_eq_u32 s86, 0", "s_cbranch_scc1 L_tail_%="]
    out += ["L_top_%=:"] + text("body0") + text("body1") + ["s_cbranch_scc1 L_top_%="]
    out += ["L_tail_%=:"] + text("tail0") + text("tail1")
    out += ["s_nop 7", "s_nop 7"]
    for t in range(f.T):
        out += [it[1] for it in fold_tile(f, t)]
    out.append("s_mov_b32 m0, s90")
    body = " \\\n".join('    "%s\\n"' % l for l in out)
    clob = ", ".join('"v%d"' % r for r in range(f.ACC[0], f.END))
    clob += ", " + ", ".join('"s%d"' % r for r in range(80, 91)) + ', "scc", "memory"'
    res = "#define %s_TEXT \\\n%s\n#define %s_CLOBBERS %s\n" % (name, body, name, clob)
    for t in range(f.T):
        res += '#define %s_S%d "=&{v[%d:%d]}"\n' % (name, t, f.S[t], f.S[t] + 3)
    return res


if __name__ == "__main__":
    print("// GENERATED by tools/gen_kw_asm.py -- do not edit.  See that file for the schedule, the wait counts and the register plan.")
    print(emit(2, "APRIL_KWLOOP_M2"))
    print(emit(1, "APRIL_KWLOOP_M1"))
