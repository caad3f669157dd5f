"""Greedy search + partial/final/silence state machine (reference src/april_session.c:199-429).

The reference's april_session.c cannot be compiled here (needs onnxruntime_c_api.h), so this part of
the oracle is pinned by hand-derived expectations (scenarios below were worked out from the
reference source, line numbers in comments), and the product's host-side implementation
(april_asr_amd/csrc/session.cc `Greedy`, driven through aprilx_greedy_*) is then checked against the
oracle on thousands of random joiner results that reach every branch (G5)."""
import ctypes as C

import numpy as np
import pytest

import april_asr_amd as A
from april_asr_amd import _ffi
from oracle import orc_py as O

import blank_models as BM

PARTIAL, FINAL, SILENCE = 1, 2, 4


class ScriptedOracle:
    """Oracle session whose networks are scripted: each joiner call pops the next (idx, max, blank)."""

    def __init__(self, model_path, triples):
        self.L = O.lib()
        self.f = self.L.orc_file_open(model_path.encode())
        self.P = self.f.contents.params
        self.V = self.P.token_count
        self.triples = list(triples)
        self.pos = 0
        self.events = []

        def enc(ud, x, h, c, e, h2, c2):
            pass

        def dec(ud, ctx, dout):
            pass

        def joi(ud, e, d, logits):
            idx, mx, bl = self.triples[self.pos] if self.pos < len(self.triples) else (1, -50.0, 50.0)
            self.pos += 1
            for i in range(self.V):
                logits[i] = -1000.0
            logits[idx] = mx
            logits[self.P.blank_id] = bl

        self._fns = (O.ENC_FN(enc), O.DEC_FN(dec), O.JOI_FN(joi))
        self.nets = O.OrcNets(None, *self._fns)

        def handler(ud, typ, count, toks):
            self.events.append((int(typ), [(int(toks[i].id), float(toks[i].logprob), int(toks[i].flags), int(toks[i].time_ms))
                                           for i in range(count)]))
        self._h = O.HANDLER(handler)
        self.s = self.L.orc_session_new_scripted(C.byref(self.P), C.byref(self.nets), 1, 8, 8, 8, self.V, self._h, None)

    def run_chunks(self, n_chunks, flush=False):
        n = 640 * n_chunks + 1152          # chunk j needs 640 j + 1792 samples
        pcm = np.zeros(n, np.int16)
        self.L.orc_session_feed_pcm16(self.s, pcm.ctypes.data, n)
        assert self.L.orc_session_chunks(self.s) == n_chunks
        if flush:
            self.L.orc_session_flush(self.s)
        return int(self.L.orc_session_chunks(self.s))

    def close(self):
        self.L.orc_session_free(self.s)
        self.L.orc_file_free(self.f)


def run_product(model, triples, n_chunks, finish):
    L = _ffi.lib()
    ev = []
    tok_index = {}
    for i in range(model.dims.vocab):
        tok_index[model.token(i).encode()] = i

    def handler(ud, typ, count, toks):
        ev.append((int(typ), [(tok_index[toks[i].token], float(toks[i].logprob), int(toks[i].flags), int(toks[i].time_ms))
                              for i in range(count)]))
    h = _ffi.HANDLER(handler)
    g = L.aprilx_greedy_create(model._handle, h, None)
    pos, now = 0, 0
    ctx = (C.c_int32 * 2)()
    for _ in range(n_chunks):
        now += 40
        for r in range(3):
            idx, mx, bl = triples[pos] if pos < len(triples) else (1, -50.0, 50.0)
            pos += 1
            if L.aprilx_greedy_step(g, idx, mx, bl, 1.0 if r == 0 else 0.0, now, ctx):
                break
    if finish:
        L.aprilx_greedy_finish(g)
    L.aprilx_greedy_free(g)
    return ev, pos


def tok(tokens, text):
    return tokens.index(text)


def test_hand_derived_plain_and_provisional(built, tiny_model):
    T = tiny_model["tokens"]
    w1 = next(i for i, t in enumerate(T) if t.startswith(" ") and len(t) > 2)         # a word-start token
    c1 = next(i for i, t in enumerate(T) if not t.startswith(" ") and t.isalpha() and len(t) > 1)
    c2 = next(i for i, t in enumerate(T) if not t.startswith(" ") and t.isalpha() and len(t) > 1 and i != c1)
    tr = [
        (w1, 5.0, 0.0),      # chunk 1 r0: non-blank (0-1 > 5 false)          -> PARTIAL [w1]           (:361-400)
        (c1, 0.0, 10.0),     # chunk 1 r1: blank; M'=0 > 6? no; head unchanged -> nothing               (:401-426)
        (c1, 7.0, 10.0),     # chunk 2 r0: blank (9 > 7); M'=7-40/3000 > 6     -> provisional PARTIAL [w1, c1(-1)]
        (c1, 7.0, 10.0),     # chunk 3: same provisional token, nothing else changed -> suppressed        (:272-276)
        (c2, 7.5, 10.0),     # chunk 4: different provisional token               -> PARTIAL [w1, c2(-0.5)]
        (c2, 0.0, 10.0),     # chunk 5: not confident; last_call_head(2) != head(1) -> PARTIAL [w1]       (:287-291)
        (c2, 0.0, 10.0),     # chunk 6: nothing
    ]
    o = ScriptedOracle(tiny_model["path"], tr)
    o.run_chunks(6)
    ev = o.events
    assert [e[0] for e in ev] == [PARTIAL] * 4
    assert ev[0][1] == [(w1, 5.0, 1, 40)]
    assert ev[1][1] == [(w1, 5.0, 1, 40), (c1, -1.0, 0, 80)]
    assert ev[2][1] == [(w1, 5.0, 1, 40), (c2, -0.5, 0, 160)]
    assert ev[3][1] == [(w1, 5.0, 1, 40)]
    o.close()


def test_hand_derived_silence_and_flush(built, tiny_model):
    T = tiny_model["tokens"]
    w1 = next(i for i, t in enumerate(T) if t.startswith(" ") and len(t) > 2)
    c1 = next(i for i, t in enumerate(T) if not t.startswith(" ") and t.isalpha() and len(t) > 1)
    # chunk 1: two tokens then blank; then 55 blank chunks: silence fires at the first chunk with gap >= 2200 ms
    tr = [(w1, 5.0, 0.0), (c1, 4.0, 0.0), (c1, 0.0, 10.0)] + [(c1, -20.0, 10.0)] * 60
    o = ScriptedOracle(tiny_model["path"], tr)
    o.run_chunks(57)
    ev = o.events
    # PARTIAL[w1], PARTIAL[w1,c1], then at t = 40 + 2200 = 2240 ms (chunk 56): FINAL + SILENCE, once (:414-417,257-268)
    assert [e[0] for e in ev] == [PARTIAL, PARTIAL, FINAL, SILENCE]
    assert ev[2][1] == [(w1, 5.0, 1, 40), (c1, 4.0, 0, 40)]
    assert ev[3][1] == []
    # flush afterwards: nothing active, silence already emitted -> no more callbacks (:547-564)
    o.L.orc_session_flush(o.s)
    assert len(o.events) == 4
    o.close()


def test_hand_derived_punctuation_and_digits(built, tiny_model):
    T = tiny_model["tokens"]
    dot, comma, one = tok(T, "."), tok(T, ","), tok(T, "2")      # the digit test looks at text[0] (:347), so " 1" would not count
    w1 = next(i for i, t in enumerate(T) if t.startswith(" ") and len(t) > 2 and not t[1].isdigit())
    w2 = next(i for i, t in enumerate(T) if t.startswith(" ") and len(t) > 2 and not t[1].isdigit() and i != w1)
    tr = [
        (w1, 5.0, 0.0),      # c1 r0 -> PARTIAL [w1]
        (dot, 7.0, 10.0),    # c1 r1: blank by logits, but punctuation override 7 > 10-3.5 (:356-358) -> "." emitted with SENTENCE_END
        (w2, 5.0, 0.0),      # c1 r2: word boundary after a sentence end -> FINAL [w1 .] then PARTIAL [w2]   (:369-388)
        (one, 5.0, 0.0),     # c2 r0 -> PARTIAL [w2, "2"]
        (dot, 7.0, 10.0),    # c2 r1: "." after a digit is NOT punctuation (:345-351): no override -> blank, provisional "." (7 > 6)
        (comma, 7.0, 10.0),  # c3 r0: comma is punctuation but not sentence end -> override -> emitted, flags 0
        (comma, 9.0, 10.0),  # c3 r1: same as previous token -> no override (:356 !is_equal_to_previous), blank, not "confident" (same)
    ]
    o = ScriptedOracle(tiny_model["path"], tr)
    o.run_chunks(3)
    ev = o.events
    kinds = [e[0] for e in ev]
    assert kinds == [PARTIAL, PARTIAL, FINAL, PARTIAL, PARTIAL, PARTIAL, PARTIAL]
    assert ev[1][1][-1] == (dot, 7.0, 2, 40)
    assert [t[0] for t in ev[2][1]] == [w1, dot]
    assert [t[0] for t in ev[3][1]] == [w2]
    assert [t[0] for t in ev[4][1]] == [w2, one]
    assert ev[5][1][-1] == (dot, -1.0, 0, 80)             # provisional, no SENTENCE_END flag after a digit
    assert [t[0] for t in ev[6][1]] == [w2, one, comma] and ev[6][1][-1][2] == 0
    o.close()


def random_triples(rng, vocab, n, special_ids, blank=0):
    """`blank`: the id no triple names as its token.  The draws are those of blank = 0 (1 .. vocab - 1), mapped onto the ids without
    the blank, so the default sequences are what they always were."""
    def tok():
        i = int(rng.randint(1, vocab))
        return i if blank == 0 or i > blank else i - 1
    out = []
    prev = 1 if blank != 1 else 0
    while len(out) < n:
        mode = rng.randint(0, 10)
        if mode == 0:                                   # long silence
            out += [(tok(), float(rng.uniform(-30, -10)), float(rng.uniform(5, 10)))] * int(rng.randint(50, 70))
            continue
        if mode == 1:                                   # burst of tokens without word boundaries is possible (overflow path)
            for _ in range(int(rng.randint(5, 90))):
                out.append((tok(), float(rng.uniform(2, 8)), float(rng.uniform(-5, 1))))
            continue
        idx = prev if rng.rand() < 0.25 else (int(rng.choice(special_ids)) if rng.rand() < 0.3 else tok())
        prev = idx
        bl = float(rng.uniform(-2, 12))
        mx = bl + float(rng.choice([-6, -4.2, -3.8, -3.4, -1.2, -0.8, -0.2, 0.2, 3.0])) + float(rng.uniform(-0.1, 0.1))
        out.append((idx, mx, bl))
    return out


@pytest.mark.parametrize("seed,which", BM.params([0, 1, 2, 3], [0, 1, 2, 3], [("blank39", [0])]))
def test_product_greedy_matches_oracle(built, request, seed, which):
    info = BM.model_info(which, request)
    host_model = A.Model.load_host_only(info["path"])
    assert host_model.dims.blank_id == info["blank"]
    rng = np.random.RandomState(seed)
    special = [info["tokens"].index(t) for t in (".", ",", "?", "!", " 1", "2", " 3", "4")]
    triples = random_triples(rng, len(info["tokens"]), 4000, special, blank=info["blank"])
    assert all(t[0] != info["blank"] for t in triples)
    n_chunks = 1200
    o = ScriptedOracle(info["path"], triples)
    total = o.run_chunks(n_chunks, flush=True)
    got, used = run_product(host_model, triples, total, finish=True)
    assert used == o.pos
    kinds = {e[0] for e in o.events}
    assert {PARTIAL, FINAL, SILENCE} <= kinds
    assert len(got) == len(o.events)
    for a, b in zip(o.events, got):
        assert a == b
    o.close()
    host_model.close()
