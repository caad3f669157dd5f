"""The text-corpus language model inside the device search (aprilx_session_set_lm).

The statement of the contract is tests/lm_ref.py, pinned to the builder and the host's walk by tests/test_lm_cpu.py.  Here: the decision
kernel's LM forms on given rows (rows with and without a model, with a boosting set, a strict set, search options and alternatives in one
launch; rows built so that one lane decides), live sessions reproduced from their own traced logits in the three feeding modes, the life
cycle and its structural zeros, and the refusals that need a live session."""
import ctypes as C

import numpy as np
import pytest

import bias_ref as BR
import bias_strict_ref as SR
import blank_models as BM
import confidence_ref as CR
import lm_ref as R
import lm_worker as W
import search_options_ref as SO
from conftest import speech_like_pcm

pytestmark = pytest.mark.gpu
VALID, BLANK, CTX = 1, 2, 4
SIZES = dict(tiny=(40, 0), medium=(131, 0), blank39=(40, 39), blank255=(500, 255), blank256=(500, 256))


def load(which, request):
    import april_asr_amd as A
    gm = A.Model(BM.model_info(which, request)["path"])
    assert (gm.dims.vocab, gm.dims.blank_id) == SIZES[which]
    return gm


def session_pcm():
    return np.concatenate([speech_like_pcm(3.0, seed=12, silence=(1.5, 1.9)), np.zeros(16000 * 3, np.int16), speech_like_pcm(2.0, seed=13)])


def session_corpus(texts, blank, seed=3):
    """20 lines made of the model's own token texts"""
    return W.corpus_of(W.token_lines(texts, blank, np.random.default_rng(seed), 20))


# ---------------------------------------------------------------- 1. given rows
class Fix:
    """one model with a language model, a boosting set and a strict set, and the statement's objects for all three"""

    def __init__(self, gm, order=5, w=0.7, b=0.4, pool_every=1):
        self.gm, self.w, self.b = gm, w, b
        self.texts, self.blank = W.texts_of(gm), gm.dims.blank_id
        self.V = gm.dims.vocab
        self.cls = SO.token_classes(self.texts)
        rng = np.random.default_rng(self.V * 7 + self.blank)
        ids = [i for i, t in enumerate(self.texts) if i != self.blank and t]
        pool = [i for i in ids if i % pool_every == 0]
        self.lines = W.token_lines(self.texts, self.blank, rng, 20, pool=pool)
        body = W.corpus_of(self.lines)
        self.seen = set(body) | {0x20}
        self.lm, self.ref = gm.lm(body, order), R.LmRef(self.texts, self.blank, body, order)
        W.same_model(self.lm, self.ref)
        phrases = [(self.lines[i], float(np.float32(rng.uniform(0.5, 3.0)))) for i in range(6)]
        self.boost, self.boost_ref = gm.bias(phrases), BR.BiasRef(self.texts, self.blank, phrases)
        self.strict, self.strict_ref = gm.bias(phrases, strict=True), SR.StrictRef(self.texts, self.blank, phrases)
        self.deep = [s for s, h in enumerate(self.ref.ctx) if len(h) == order - 1]

    def close(self):
        for x in (self.lm, self.boost, self.strict):
            x.close()


def check_launch(fx, rows, logits, ee, rnd, bias=None, what=""):
    """rows: dicts(node=-1|n, trie=-1|s, opts=None|(E, p), state=[4], now).  One launch of the LM forms against the statement on every
    bit of idx, max_val, blank_val, flags, search state, node and trie state.  Returns the records and the compared rows."""
    n = len(rows)
    bias_h, bias_ref = (None, None) if bias is None else ((fx.boost, fx.boost_ref) if bias == "boost" else (fx.strict, fx.strict_ref))
    opts = [r.get("opts") for r in rows]
    rec, st, bs, ls = fx.gm.run_decide_lm(logits, ee, [r["now"] for r in rows], rnd, [r["state"] for r in rows], fx.lm, [r["node"] for r in rows],
                                          fx.w, fx.b, opts=opts if any(o is not None for o in opts) else None, bias=bias_h,
                                          bias_state=[r.get("trie", -1) for r in rows] if bias_h is not None else None)
    compared = []
    for i, r in enumerate(rows):
        has_lm, has_bias = r["node"] >= 0, bias_ref is not None and r.get("trie", -1) >= 0
        o = r.get("opts")
        row = R.Row(fx.cls, fx.blank, fx.ref if has_lm else None, fx.w, fx.b, bias_ref if has_bias else None, (o[0], o[1], 0) if o else None)
        row.search.set_state(r["state"])
        row.node, row.trie = max(r["node"], 0), max(r.get("trie", 0), 0)
        compared.append(row.compared(logits[i]))
        idx, mx, bl, is_blank, silence, changed = row.step(logits[i], ee, r["now"])
        flags = VALID | (BLANK if is_blank else 0) | (CTX if changed else 0)
        tag = "%s row %d %r" % (what, i, {k: r[k] for k in ("node", "trie", "opts") if k in r})
        assert int(rec["idx"][i]) == idx, (tag, int(rec["idx"][i]), idx)
        assert W.bits(rec["max"][i]) == W.bits(mx) and W.bits(rec["blank"][i]) == W.bits(bl), (tag, rec[i], mx, bl)
        assert int(rec["flags"][i]) == flags, (tag, int(rec["flags"][i]), flags)
        assert [int(x) for x in st[i]] == row.search.state(), (tag, list(st[i]), row.search.state())
        assert int(ls[i]) == (row.node if has_lm else -1), (tag, "node", int(ls[i]), row.node)
        if bias_h is not None:
            assert int(bs[i]) == (row.trie if has_bias else -1), (tag, "trie", int(bs[i]), row.trie)
    return rec, compared


def mixed_rows(fx, rng, n=9):
    """no model / a model / a model with a set / a model with options / deepest node / start, with search states that reach every branch"""
    ids = [i for i in range(fx.V) if i != fx.blank]
    rows = []
    for i in range(n):
        kind = i % 9
        a, b = int(rng.choice(ids)), int(rng.choice(ids))
        state = [[fx.blank, fx.blank, -1, 0], [a, b, b, 40], [fx.blank, a, a, 0]][i % 3]
        r = dict(node=-1, trie=-1, state=state, now=int(rng.choice([40, 80, 500, 2300, 4000])))
        if kind >= 1:
            r["node"] = fx.ref.start if kind in (1, 8) else (int(rng.choice(fx.deep)) if kind in (2, 7) else int(rng.integers(0, fx.ref.nodes)))
        if kind in (3, 4, 7):
            r["trie"] = 0 if kind == 3 else -2          # -2: replaced by a state of the launch's set
        if kind in (5, 7):
            r["opts"] = (400, 1.5) if kind == 5 else (3000, -0.5)
        rows.append(r)
    return rows


@pytest.mark.parametrize("which", ["tiny", "medium", "blank39", "blank255", "blank256"])
def test_mixed_rows_in_one_launch(which, request):
    """V = 40, 131 and 500; blank ids 39 of 40, 255 and 256 of 500; 9 rows per launch; round 0 and round 2; with a boosting set and with a
    strict set; rows without a model equal aprilx_run_decide bit for bit"""
    gm = load(which, request)
    fx = Fix(gm)
    rng = np.random.default_rng(fx.V)
    decided = {"blank": 0, "token": 0, "silence": 0, "moved": 0}
    for bias in (None, "boost", "strict"):
        bref = {None: None, "boost": fx.boost_ref, "strict": fx.strict_ref}[bias]
        for rnd in (0, 2):
            for trial in range(3):
                rows = mixed_rows(fx, rng)
                for r in rows:
                    if r["trie"] == -2:
                        r["trie"] = int(rng.integers(0, bref.S)) if bref is not None else -1
                logits = rng.normal(0.0, 3.0, (len(rows), fx.V)).astype(np.float32)
                logits[:, fx.blank] += np.float32(rng.choice([-6.0, 0.0, 9.0], len(rows)))
                if trial == 2:                                      # the LM term must not rescue a NaN row, nor poison another
                    logits[1, :] = np.nan
                rec, _ = check_launch(fx, rows, logits, 1.0 if rnd == 0 else 0.0, rnd, bias, "%s %s round %d" % (which, bias, rnd))
                decided["blank"] += int(((rec["flags"] & BLANK) != 0).sum()); decided["token"] += int(((rec["flags"] & BLANK) == 0).sum())
                # a row without a model (and without a set): the record aprilx_run_decide gives
                st = np.ascontiguousarray([rows[0]["state"]], np.int32); plain = np.zeros(1, rec.dtype); now = np.array([rows[0]["now"]], np.int32)
                lg0 = np.ascontiguousarray(logits[:1])
                assert gm._L.aprilx_run_decide(gm._handle, 1, 0, lg0.ctypes.data, C.c_float(1.0 if rnd == 0 else 0.0), now.ctypes.data, rnd, st.ctypes.data, plain.ctypes.data) == 0
                assert rec[0].tobytes() == plain[0].tobytes()
    assert decided["blank"] > 20 and decided["token"] > 20
    # the end-of-flush reset (op 1): rows with a model return to its start node, the others stay without one
    _, st, _, ls = gm.run_decide_lm(np.zeros((3, fx.V), np.float32), 0.0, [0, 0, 0], 0, [[5, 6, 6, 7], [fx.blank, fx.blank, -1, 0], [5, 6, 6, 7]], fx.lm,
                                    [fx.deep[-1], -1, 0], fx.w, fx.b, op=1)
    assert list(ls) == [fx.ref.start, -1, fx.ref.start] and list(st[0]) == [fx.blank, fx.blank, -1, 7] and fx.ref.start != 0
    fx.close(); gm.close()


@pytest.mark.parametrize("which", ["tiny", "blank255"])
def test_confidences_on_the_fused_row(which, request):
    """K = 4 alternatives on rows with and without a model, with a boosting and a strict set: ids exact, logits the compared bits (alt 0 is
    the record's idx / max_val), lse inside section 12's bound over the blank and the tokens that took part"""
    gm = load(which, request)
    fx = Fix(gm)
    rng = np.random.default_rng(fx.V + 1)
    for bias in (None, "boost", "strict"):
        bref = {None: None, "boost": fx.boost_ref, "strict": fx.strict_ref}[bias]
        bias_h = {None: None, "boost": fx.boost, "strict": fx.strict}[bias]
        n = 9
        nodes = [-1, fx.ref.start, fx.deep[0], 0] + [int(x) for x in rng.integers(0, fx.ref.nodes, n - 4)]
        tries = [(-1 if i % 3 == 0 else int(rng.integers(0, bref.S))) if bref is not None else -1 for i in range(n)]
        logits = rng.normal(0.0, 3.0, (n, fx.V)).astype(np.float32)
        info = gm.run_confidence_lm(logits, 4, fx.lm, nodes, fx.w, fx.b, bias=bias_h, bias_state=tries if bias_h is not None else None)
        rows = [dict(node=nodes[i], trie=tries[i], state=[fx.blank, fx.blank, -1, 0], now=0) for i in range(n)]
        rec, compared = check_launch(fx, rows, logits, 1.0, 0, bias, "conf " + str(bias))
        for i in range(n):
            has_bias = bref is not None and tries[i] >= 0
            strict = has_bias and bias == "strict"
            ids = bref.permitted(tries[i]) if strict else [t for t in range(fx.V) if t != fx.blank]
            lse64, alt, alt_v, n_alt = R.confidence(compared[i], ids, fx.blank, 4)
            o = info[i]
            assert int(o.n_alt) == n_alt and [int(o.alt_id[k]) for k in range(n_alt)] == [int(x) for x in alt], (bias, i)
            got = np.array([o.alt_logit[k] for k in range(n_alt)], np.float32)
            assert np.array_equal(W.bits(got), W.bits(alt_v)), (bias, i, got, alt_v)
            if n_alt == 0:                                # nothing permitted beat the initial value: the record says so, the lse is a NaN
                assert int(rec["idx"][i]) == -1 and np.isnan(o.lse)
                continue
            assert int(o.alt_id[0]) == int(rec["idx"][i]) and W.bits(o.alt_logit[0]) == W.bits(rec["max"][i])
            assert abs(float(o.lse) - lse64) <= CR.lse_bound(lse64), (bias, i, float(o.lse), lse64)
            want_bl = float(np.float32(logits[i, fx.blank])) - lse64
            assert abs(float(o.blank_logprob) - want_bl) <= CR.ls_bound(lse64, want_bl)
    fx.close(); gm.close()


def test_rows_one_lane_decides(request):
    """V = 500, blank 255: tokens n and n + 256 are compared by ONE lane.  Equal logits the model separates, the same pair with w = 0 (the
    lower id wins), a tie on v' the model creates between unequal logits, a forbidden token the model would prefer, the deepest node and
    the start node, and a token whose walk backs off to the root and pays unk_logp."""
    gm = load("blank255", request)
    fx = Fix(gm, pool_every=3)                   # a third of the tokens make the corpus: bytes of the others stay unseen
    V, blank, ref = fx.V, fx.blank, fx.ref
    base = dict(state=[blank, blank, -1, 0], now=40)

    def row(**kw):
        r = np.full(V, -1000.0, np.float32)
        r[blank] = -50.0
        for k, v in kw.items():
            r[int(k[1:])] = v
        return r

    for node in (ref.start, fx.deep[0], fx.deep[-1]):
        pair = next((n, n + 256) for n in range(0, V - 256) if n != blank and n + 256 != blank and W.bits(ref.term(node, n, fx.w, fx.b)) != W.bits(ref.term(node, n + 256, fx.w, fx.b)))
        lo, hi = pair
        want = lo if ref.term(node, lo, fx.w, fx.b) > ref.term(node, hi, fx.w, fx.b) else hi
        rec, _ = check_launch(fx, [dict(base, node=node)], row(**{"t%d" % lo: 4.0, "t%d" % hi: 4.0})[None], 1.0, 0, None, "pair the model separates")
        assert int(rec["idx"][0]) == want
    # the model prefers the HIGHER id of some pair at some node, so that the lane's second comparison must replace the first
    found = None
    for node in [ref.start] + fx.deep:
        for n in range(0, V - 256):
            if n != blank and n + 256 != blank and ref.term(node, n + 256, fx.w, fx.b) > ref.term(node, n, fx.w, fx.b):
                found = (node, n); break
        if found:
            break
    assert found
    node, n = found
    rec, _ = check_launch(fx, [dict(base, node=node)], row(**{"t%d" % n: 4.0, "t%d" % (n + 256): 4.0})[None], 1.0, 0, None, "higher id preferred")
    assert int(rec["idx"][0]) == n + 256
    # w = 0, b = 0: term = 0 * score + 0 for both, the lower index must win
    w, b = fx.w, fx.b
    fx.w, fx.b = 0.0, 0.0
    rec, _ = check_launch(fx, [dict(base, node=node)], row(**{"t%d" % n: 4.0, "t%d" % (n + 256): 4.0})[None], 1.0, 0, None, "w = 0")
    assert int(rec["idx"][0]) == n
    fx.w, fx.b = w, b
    # a tie on v' between unequal logits: v[q] is searched ulp by ulp until v[q] + term_q has the bits of v[p] + term_p
    p, q = n, n + 256
    tp, tq = ref.term(node, p, w, b), ref.term(node, q, w, b)
    target = np.float32(np.float32(4.0) + tp)
    vq = np.float32(target - tq)
    for _ in range(64):
        got = np.float32(vq + tq)
        if W.bits(got) == W.bits(target):
            break
        vq = np.nextafter(vq, np.float32(np.inf if got < target else -np.inf), dtype=np.float32)
    assert W.bits(np.float32(vq + tq)) == W.bits(target) and W.bits(vq) != W.bits(np.float32(4.0))
    rec, _ = check_launch(fx, [dict(base, node=node)], row(**{"t%d" % p: 4.0, "t%d" % q: vq})[None], 1.0, 0, None, "tie the model creates")
    assert int(rec["idx"][0]) == p and W.bits(rec["max"][0]) == W.bits(target)
    # a forbidden token the model would prefer: the strict set's root permits few tokens; a forbidden one gets the best logit and term
    permitted = set(fx.strict_ref.permitted(0))
    forb = max((t for t in range(V) if t != blank and t not in permitted), key=lambda t: float(ref.term(ref.start, t, w, b)))
    ok = sorted(permitted)[0]
    rec, _ = check_launch(fx, [dict(base, node=ref.start, trie=0)], row(**{"t%d" % forb: 30.0, "t%d" % ok: 1.0})[None], 1.0, 0, "strict", "forbidden token")
    assert int(rec["idx"][0]) in permitted and int(rec["idx"][0]) != forb
    # a token whose walk backs off to the root and takes unk: its first byte was never seen
    unk = next(t for t in range(V) if t != blank and fx.texts[t] and fx.texts[t][0] not in fx.seen)
    for node in (fx.deep[-1], ref.start):
        rec, _ = check_launch(fx, [dict(base, node=node)], row(**{"t%d" % unk: 60.0})[None], 1.0, 0, None, "unk")
        assert int(rec["idx"][0]) == unk and not (rec["flags"][0] & BLANK)
        s, acc = node, np.float32(0.0)
        path = []
        while ref._arc[s].get(fx.texts[unk][0]) is None and s != 0:
            path.append(s); s = int(ref.back[s])
        assert s == 0 and ref._arc[0].get(fx.texts[unk][0]) is None and len(path) >= 1
    fx.close(); gm.close()


# ---------------------------------------------------------------- 2. live sessions from their own traced logits
def run_session(gm, pcm, feed, lm=None, w=0.5, b=2.0, mode="sync", trace=False, twin=False, k=None, bias=None, opts=None):
    """One session with the model (and, with `twin`, an identical one without in the same engine) over `pcm`, then a flush.
    Returns (events, traced logits, chunks, twin events, info log)."""
    import april_asr_amd as A
    ev, ev2 = [], []
    kw = dict(raw_events=True, asynchronous=(mode == "async"))
    o = dict(endpoint_silence_ms=opts[0], blank_penalty=opts[1]) if opts else {}
    s = A.Session(gm, lambda t, toks: ev.append((t, toks)), lm=lm, lm_weight=w, lm_token_bonus=b, alternatives=k, bias=bias, **kw, **o)
    s.info_log = [] if k else None
    ss = [s]
    if twin:
        ss.append(A.Session(gm, lambda t, toks: ev2.append((t, toks)), **kw))
    if trace:
        s.trace_logits(20000)
    g = A.SessionGroup(ss)
    start = lm.start if lm is not None else 0
    assert s.lm_state() == (start, start)
    for i in range(0, pcm.size, feed):
        if mode == "pipelined":
            g.feed_pipelined([pcm[i:i + feed]] * len(ss), depth=2)
        else:
            for x in ss:
                x.feed_pcm16(pcm[i:i + feed])
            h, d = s.lm_state()                       # (waits until the session is idle, also in async mode)
            assert h == d, "node: host %d, device %d after the feed at sample %d" % (h, d, i)
    if mode == "pipelined":
        g.drain()
        h, d = s.lm_state()
        assert h == d
    for x in ss:
        x.flush()
    assert s.lm_state() == (start, start), "after a flush the node must read start"
    out = (ev, s.traced_logits().copy() if trace else None, s.chunks(), ev2, s.info_log)
    for x in ss:
        x.close()
    return out


def replay(gm, texts, row, lg, chunks, stride_ms=40):
    """the session again from its raw traced logits: the statement decides (lm_ref.Row), the library's host state machine turns the
    decisions into callbacks"""
    from april_asr_amd import _ffi
    L = gm._L
    ev = []

    def on(ud, t, n, toks):
        ev.append((int(t), [(toks[i].token, float(toks[i].logprob), int(toks[i].flags), int(toks[i].time_ms)) for i in range(n)]))
    cb = _ffi.HANDLER(on)
    g = L.aprilx_greedy_create(gm._handle, cb, None)
    if row.search.opts is not None:
        from search_options_worker import make_options
        assert L.aprilx_greedy_set_search_options(g, C.byref(make_options(row.search.opts))) == 0
    r_i, nodes = 0, []
    for c in range(1, chunks + 1):
        for r in range(3):
            assert r_i < len(lg), "fewer traced evaluations than the search needs"
            ee = 1.0 if r == 0 else 0.0
            nodes.append(row.node)
            idx, mx, bl, is_blank, _, _ = row.step(lg[r_i], ee, c * stride_ms)
            got = L.aprilx_greedy_step(g, idx, float(mx), float(bl), ee, c * stride_ms, None)
            assert bool(got) == is_blank
            r_i += 1
            if is_blank:
                break
    assert r_i == len(lg), "the session evaluated %d rows, the statement's search %d" % (len(lg), r_i)
    L.aprilx_greedy_finish(g)
    L.aprilx_greedy_free(g)
    return ev, nodes


def same_events(a, b):
    assert len(a) == len(b), (len(a), len(b))
    for (t0, k0), (t1, k1) in zip(a, b):
        assert t0 == t1 and len(k0) == len(k1)
        for x, y in zip(k0, k1):
            assert x[0] == y[0] and x[2:] == y[2:], (x, y)
            assert W.bits(x[1]) == W.bits(y[1]), (x, y)


@pytest.mark.parametrize("which", ["tiny", "blank39"])
def test_live_sessions(which, request):
    """sync, async and pipelined: delivered tokens and logprob bits equal the statement run over the session's traced logits; the node
    agrees between host and device after every feed and reads start after the flush; replay_mismatch stays 0; an identical twin without a
    model in the same engine delivers what it delivers in an engine nobody opted into"""
    import april_asr_amd as A
    path = BM.model_info(which, request)["path"]
    pcm = session_pcm()
    gm0 = A.Model(path)
    plain = run_session(gm0, pcm, 1600)[0]
    assert gm0.lm_stats() == (0, 0, 0)
    gm0.close()
    gm = A.Model(path)
    texts, blank = W.texts_of(gm), gm.dims.blank_id
    body = session_corpus(texts, blank)
    lm, ref = gm.lm(body, 5), R.LmRef(texts, blank, body, 5)
    cls = SO.token_classes(texts)
    w, b = 0.5, 8.0                                    # (a bonus large enough that the synthetic network's blank does not win every round)
    ev, lg, chunks, _, _ = run_session(gm, pcm, 1600, lm, w, b, trace=True)
    want, nodes = replay(gm, texts, R.Row(cls, blank, ref, w, b), lg, chunks)
    same_events(ev, want)
    n_tok = sum(len(t) for _, t in ev)
    assert n_tok > 0 and len({x for x in nodes}) > 3, "the run must deliver tokens and move through the automaton"
    for mode in ("sync", "async", "pipelined"):
        ev_m, _, _, twin, _ = run_session(gm, pcm, 1600, lm, w, b, mode=mode, twin=True)       # untraced: the captured graphs
        same_events(ev_m, want)
        same_events(twin, plain)
    assert ev != plain, "the model must change this transcript"
    assert gm.stats().replay_mismatch == 0
    lm.close(); gm.close()


def test_model_strict_set_options_and_alternatives_at_once(request):
    import april_asr_amd as A
    gm = A.Model(BM.model_info("tiny", request)["path"])
    texts, blank = W.texts_of(gm), gm.dims.blank_id
    rng = np.random.default_rng(9)
    lines = W.token_lines(texts, blank, rng, 20)
    body = W.corpus_of(lines)
    lm, ref = gm.lm(body, 4), R.LmRef(texts, blank, body, 4)
    phrases = [(x, 1.0) for x in lines[:8]]
    strict, sref = gm.bias(phrases, strict=True), SR.StrictRef(texts, blank, phrases)
    opts = (600, 2.0)
    pcm = session_pcm()
    ev, lg, chunks, _, info = run_session(gm, pcm, 1600, lm, 0.4, 1.0, trace=True, k=4, bias=strict, opts=opts)
    row = R.Row(SO.token_classes(texts), blank, ref, 0.4, 1.0, sref, (opts[0], opts[1], 0))
    want, _ = replay(gm, texts, row, lg, chunks)
    same_events(ev, want)
    pieces = {texts[n] for e in sref.eff for n in e}
    assert sum(len(t) for _, t in ev) > 0 and {t[0] for _, toks in ev for t in toks} <= pieces
    # every delivered token's first alternative is the token itself with the logprob the search compared
    seen = 0
    for (typ, toks), (_, infos) in zip(ev, info):
        for t, raw in zip(toks, infos):
            if raw is None:
                continue
            from april_asr_amd import _ffi
            o = _ffi.AprilxTokenInfo.from_buffer_copy(raw)
            assert texts[int(o.alt_id[0])] == t[0] and 1 <= int(o.n_alt) <= 4
            seen += 1
    assert seen > 0 and gm.stats().replay_mismatch == 0
    lm.close(); strict.close(); gm.close()


# ---------------------------------------------------------------- 3. structure and refusals
def test_life_cycle_and_structural_zeros(request, capfd):
    import april_asr_amd as A
    gm = A.Model(BM.model_info("tiny", request)["path"])
    texts, blank = W.texts_of(gm), gm.dims.blank_id
    pcm = session_pcm()[:16000]
    run_session(gm, pcm, 1600)
    assert gm.lm_stats() == (0, 0, 0), "an engine without an opted-in session launches none of the new forms"
    lm = gm.lm(session_corpus(texts, blank), 5)
    ev = []
    s1 = A.Session(gm, lambda t, toks: ev.append(t), lm=lm)
    s2 = A.Session(gm, lambda t, toks: ev.append(t), lm=lm, lm_weight=0.0)
    for s in (s1, s2):
        s.feed_pcm16(pcm[:3200])
    launches, resident, uploads = gm.lm_stats()
    assert launches > 0 and (resident, uploads) == (1, 1), "two sessions sharing one model upload it once"
    # a model mid-stream is refused (the rule of aprilx_session_set_input_rate); after a completed flush it is accepted
    capfd.readouterr()
    with pytest.raises(ValueError):
        s1.set_lm(None)
    with pytest.raises(ValueError):
        s1.set_lm(lm, 0.2)
    assert "refused" in capfd.readouterr().err
    s1.flush()
    s1.set_lm(lm, 0.2)
    assert s1.lm_state() == (lm.start, lm.start)
    # snapshot and restore with a model are refused with a message
    with pytest.raises(RuntimeError):
        s1.snapshot()
    assert "language model" in capfd.readouterr().err
    donor = A.Session(gm, lambda t, toks: None)
    blob = donor.snapshot()
    fresh = A.Session(gm, lambda t, toks: None, lm=lm)
    with pytest.raises(ValueError, match="language model"):
        fresh.restore(blob)
    fresh.set_lm(None)
    fresh.restore(blob)                                   # without the model the same blob is accepted
    for bad in ((float("nan"), 0.0), (-0.1, 0.0), (10.5, 0.0), (0.3, float("inf"))):
        with pytest.raises(ValueError):
            donor.set_lm(lm, *bad)
    assert donor.lm_state() == (0, 0)
    # another token list
    gm2 = A.Model(BM.model_info("blank39", request)["path"])
    other = A.Session(gm2, lambda t, toks: None)
    with pytest.raises(ValueError):
        other.set_lm(lm)
    assert "another token list" in capfd.readouterr().err
    other.close(); gm2.close()
    # after the last session with the model is released, the model is no longer resident
    for s in (s1, s2, fresh, donor):
        s.close()
    run_session(gm, pcm[:3200], 1600)                     # (a flight: the stepping thread applies the queued releases)
    assert gm.lm_stats()[1:] == (0, 1)
    # ... and the next first use uploads it again
    run_session(gm, pcm[:3200], 1600, lm)
    run_session(gm, pcm[:1600], 1600)
    assert gm.lm_stats()[1:] == (0, 2)
    lm.close(); gm.close()


def test_ninth_model_on_an_engine_is_refused(request, capfd):
    import april_asr_amd as A
    gm = A.Model(BM.model_info("tiny", request)["path"])
    texts, blank = W.texts_of(gm), gm.dims.blank_id
    lms = [gm.lm(session_corpus(texts, blank, seed=100 + i), 3) for i in range(9)]
    ss = [A.Session(gm, lambda t, toks: None) for _ in range(10)]
    for i in range(8):
        ss[i].set_lm(lms[i])
    ss[8].set_lm(lms[3])                                  # a model the engine holds already: shared, accepted
    capfd.readouterr()
    with pytest.raises(ValueError):
        ss[9].set_lm(lms[8])
    assert "8 other language models" in capfd.readouterr().err
    ss[0].set_lm(None)                                    # an entry is let go: once a flight has released it, the ninth model fits
    ss[0].feed_pcm16(session_pcm()[:3200]); ss[0].flush()
    ss[9].set_lm(lms[8])
    for s in ss:
        s.close()
    for x in lms:
        x.close()
    gm.close()
