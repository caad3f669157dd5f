"""Reference statement of the per-session search options, in the manner of tests/bias_ref.py: the search
decision and the result state machine in float32 numpy, written from the contract and independent of the product's code.

A session has three options; `opts` below is None (a session without options) or (E, p, U):
    E  endpoint_silence_ms  replaces 2200 in the blank branch:            now - last_emit >= E
    p  blank_penalty        bl' = bl - p (ONE fp32 subtraction) replaces bl in exactly three comparisons:
                                (bl' - ee) > tv,    tv > (bl' - 3.5),    decayed > (bl' - 4.0)
    U  max_utterance_ms     host only: a non-blank WORD_BOUNDARY token that arrives with tokens active and now - first >= U finalises them
`Search` is what the device decides (the part the next network call depends on); `Greedy` adds the callbacks the host builds from the
same three numbers.  Everything not named above -- the 3000 / 4.0 / 8.0 / 3.5 constants, the context-clear quirk, de-duplication -- is the
machine as it stands without options.  Records, token logprobs and traced logits keep the RAW blank logit."""
import numpy as np

INIT = np.float32(-9999999999.0)
PARTIAL, FINAL, SILENCE = 1, 2, 4
WORD_BOUNDARY, SENTENCE_END = 1, 2
MAX_ACTIVE = 72
f32 = np.float32


def accepted(E, p, U):
    """the values aprilx_session_set_search_options accepts"""
    return 200 <= E <= 60000 and (U == 0 or 1000 <= U <= 600000) and bool(np.isfinite(p)) and abs(p) <= 100.0


def token_classes(texts):
    out = np.zeros(len(texts), np.uint8)
    for i, t in enumerate(texts):
        t = t if isinstance(t, bytes) else t.encode()
        f = 0
        if t[:1] == b" ": f |= 1
        if len(t) == 1 and t in (b".", b"!", b"?"): f |= 2
        if t == b",": f |= 4
        if t[:1] == b".": f |= 8
        if t[:1].isdigit(): f |= 16
        out[i] = f
    return out


def argmax_record(v, blank):
    """(idx, max_val, blank_val) of the masked arg-max on one row: first maximum wins, the blank excluded, initial value -9999999999"""
    v = np.asarray(v, np.float32)
    cand = np.where(np.isnan(v), -np.inf, v).astype(np.float32)
    cand[blank] = -np.inf
    bi = int(np.argmax(cand))
    best = cand[bi]
    if not best > INIT:
        best, bi = INIT, -1
    return bi, f32(best), f32(v[blank])


def penalised(bl, opts):
    """bl': skipped entirely for a session without options; with p == 0 the bits are bl's"""
    return f32(bl) if opts is None else f32(f32(bl) - f32(opts[1]))


def endpoint_ms(opts):
    return 2200 if opts is None else int(opts[0])


class Search:
    """the device's decision: state (ctx0, ctx1, last_tok, last_emit_ms) per slot; step() returns (is_blank, silence, ctx_changed)"""

    def __init__(self, cls, blank, opts=None):
        self.cls, self.blank, self.opts = cls, blank, opts
        self.ctx = [blank, blank]
        self.last_tok = -1
        self.last_emit = 0

    def state(self):
        return [self.ctx[0], self.ctx[1], self.last_tok, self.last_emit]

    def set_state(self, st):
        self.ctx = [int(st[0]), int(st[1])]; self.last_tok = int(st[2]); self.last_emit = int(st[3])

    def step(self, idx, mx, bl, early_emit, now):
        tok, tv = int(idx), f32(mx)
        if tok < 0:
            tok, tv = (1 if self.blank == 0 else 0), INIT
        blp = penalised(bl, self.opts)
        cleared = self.ctx[1] == self.blank
        same = self.ctx[1] == tok
        ee = f32(0.0 if same else early_emit)
        is_blank = bool(f32(blp - ee) > tv)
        tc = int(self.cls[tok])
        punct = (tc & 6) != 0
        if punct and self.last_tok >= 0 and (int(self.cls[self.last_tok]) & 16) and (tc & 8):
            punct = False
        if not cleared and punct and not same and tv > f32(blp - f32(3.5)):
            is_blank = False
        silence = changed = False
        if not is_blank:
            self.last_emit = now
            self.ctx = [self.ctx[1], tok]
            self.last_tok = tok
            changed = True
        elif ((now - self.last_emit) & 0xFFFFFFFF) >= endpoint_ms(self.opts):
            silence = True
            self.last_tok = -1
            if self.ctx[0] != self.blank:
                self.ctx = [self.blank, self.blank]
                changed = True
        return is_blank, silence, changed


class Greedy:
    """the host's result state machine over the same (idx, max, blank) triples: events as (type, [(token id, logprob, flags, time_ms)])"""

    def __init__(self, cls, blank, opts=None):
        self.cls, self.blank, self.opts = cls, blank, opts
        self.ctx = [blank, blank]
        self.slot = [[-1, 0.0, 0, 0] for _ in range(MAX_ACTIVE)]     # [id, logprob, flags, time_ms]; entries behind the head keep what was last written
        self.head = 0
        self.last_call_head = 0
        self.emitted_silence = True
        self.last_emit = 0
        self.first_ms = 0
        self.events = []

    def _call(self, kind, count):
        self.events.append((kind, [tuple(t) for t in self.slot[:count]]))

    def _finalize_all(self):
        if self.head == 0:
            return
        self._call(FINAL, self.head)
        self.last_call_head = self.head
        self.head = 0

    def _finalize_before_word(self, flags):
        if self.head == 0:
            return
        if flags & WORD_BOUNDARY:
            return self._finalize_all()
        start = None
        for i in range(self.head - 1, 2, -1):
            if self.slot[i][2] & WORD_BOUNDARY:
                start = i
                break
        if start is None:
            return self._finalize_all()
        self._call(FINAL, start)
        for i in range(self.head - start):
            self.slot[i] = list(self.slot[start + i])
        self.head -= start

    def _emit_token(self, tok, force):
        if not force and self.last_call_head == self.head + 1 and self.slot[self.head][0] == tok[0]:
            return False
        self.slot[self.head] = list(tok)
        self.head += 1
        self._call(PARTIAL, self.head)
        self.last_call_head = self.head
        return True

    def step(self, idx, mx, bl, early_emit, now):
        best, best_v = int(idx), f32(mx)
        if best < 0:
            best, best_v = (1 if self.blank == 0 else 0), INIT
        blp = penalised(bl, self.opts)
        cleared = self.ctx[1] == self.blank
        same = self.ctx[1] == best
        ee = f32(0.0 if same else early_emit)
        is_blank = bool(f32(blp - ee) > best_v)
        tc = int(self.cls[best])
        flags = WORD_BOUNDARY if tc & 1 else 0
        eos = bool(tc & 2)
        punct = eos or bool(tc & 4)
        if punct and self.head > 0:
            lc = int(self.cls[self.slot[self.head - 1][0]])
            if (lc & 16) and (tc & 8):
                eos = punct = False
        if eos:
            flags |= SENTENCE_END
        if not cleared and punct and not same and best_v > f32(blp - f32(3.5)):
            is_blank = False
        if not is_blank:
            self.last_emit = now
            self.ctx = [self.ctx[1], best]
            fin = self.head >= MAX_ACTIVE - 1
            if self.head > 0 and (flags & WORD_BOUNDARY):
                prev = self.slot[self.head - 1]
                if int(self.cls[prev[0]]) & 2:
                    prev[2] |= SENTENCE_END
                    fin = True
            U = 0 if self.opts is None else int(self.opts[2])
            if U and self.head > 0 and (flags & WORD_BOUNDARY) and now - self.first_ms >= U:
                fin = True
            if fin:
                self._finalize_before_word(flags)
            if self.head >= MAX_ACTIVE - 1:
                self.head = 0
            if self.head == 0:
                self.first_ms = now
            self._emit_token((best, float(best_v), flags, now), True)
            self.emitted_silence = False
        else:
            gap = now - self.last_emit
            decayed = f32(best_v - f32(f32(gap) / f32(3000.0)))
            confident = (not same) and bool(decayed > f32(blp - f32(4.0)))
            if gap >= endpoint_ms(self.opts):
                self._finalize_all()
                if self.ctx[0] != self.blank:
                    self.ctx = [self.blank, self.blank]
                if not self.emitted_silence:
                    self.emitted_silence = True
                    self.events.append((SILENCE, []))
            elif confident:
                tok = (best, float(f32(best_v - f32(8.0))), flags, now)
                if self._emit_token(tok, False):
                    self.head -= 1
            else:
                if self.last_call_head != self.head:
                    self._call(PARTIAL, self.head)
                    self.last_call_head = self.head
        return is_blank

    def finish(self):
        self._finalize_all()
        if self.ctx[0] != self.blank:
            self.ctx = [self.blank, self.blank]
        if not self.emitted_silence:
            self.emitted_silence = True
            self.events.append((SILENCE, []))


def replay(cls, blank, opts, logits, chunks, stride_ms=40, flush_after=()):
    """A session again from its raw traced logits [evaluations][V]: up to three rounds per chunk (early_emit 1, 0, 0), the chunk ends at the
    first blank round; a flush completes behind every chunk number in `flush_after` and behind the last chunk (FINAL, context cleared,
    SILENCE; the device forgets the last token).  Returns (events, the device states after every evaluation)."""
    g, s = Greedy(cls, blank, opts), Search(cls, blank, opts)
    row, states = 0, []
    for c in range(1, chunks + 1):
        for r in range(3):
            assert row < len(logits), "fewer traced evaluations than the search needs"
            idx, mx, bl = argmax_record(logits[row], blank)
            ee = 1.0 if r == 0 else 0.0
            is_blank = g.step(idx, mx, bl, ee, c * stride_ms)
            assert s.step(idx, mx, bl, ee, c * stride_ms)[0] == is_blank
            assert s.ctx == g.ctx
            states.append(s.state())
            row += 1
            if is_blank:
                break
        if c in flush_after or c == chunks:
            g.finish()
            s.last_tok = -1
            if s.ctx[0] != blank:
                s.ctx = [blank, blank]
            assert s.ctx == g.ctx
    assert row == len(logits), "the session evaluated %d rows, the reference search %d" % (len(logits), row)
    return g.events, states
