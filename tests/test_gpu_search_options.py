"""Per-session search options inside the device search (aprilx_session_set_search_options).

The statement of the contract is tests/search_options_ref.py, pinned to the hand-derived cases of tests/golden/search_options_cases.py by
tests/test_search_options_cpu.py.  Here: the decision kernel's OPT forms on given rows (rows with and without options in one launch,
bitwise against aprilx_run_decide where the contract says so), the hand-derived cases on the device, the combination with bias sets and
confidences, live sessions reproduced from their own traced logits, the life cycle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import search_options_cases as G  # noqa: E402
import search_options_ref as R  # noqa: E402
import search_options_worker as W  # noqa: E402
import blank_models as BM  # noqa: E402
from conftest import speech_like_pcm  # noqa: E402

pytestmark = pytest.mark.gpu
VALID, BLANK, CTX = 1, 2, 4
REC = np.dtype([("idx", np.int32), ("max", np.float32), ("blank", np.float32), ("flags", np.uint32)])


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def texts_of(gm):
    return [gm._L.aprilx_model_token(gm._handle, i) or b"" for i in range(gm.dims.vocab)]


def decide_plain(gm, lg, ee, now, rnd, state):
    st = np.ascontiguousarray(state, np.int32).reshape(-1, 4).copy()
    n = st.shape[0]
    rec = np.zeros(n, REC)
    nowa = np.ascontiguousarray(now, np.int32)
    lg = np.ascontiguousarray(lg, np.float32)
    assert gm._L.aprilx_run_decide(gm._handle, n, 0, lg.ctypes.data, C.c_float(ee), nowa.ctypes.data, rnd, st.ctypes.data, rec.ctypes.data) == 0
    return rec, st


def scripted_row(V, blank, tok, mx, bl):
    r = np.full(V, -1000.0, np.float32)
    r[tok] = mx
    r[blank] = bl
    return r


@pytest.fixture(scope="module")
def tiny(tiny_model):
    import april_asr_amd as A
    gm = A.Model(tiny_model["path"])
    yield gm
    gm.close()


# ---------------------------------------------------------------- 1. given rows: with, without and with default options in one launch
@pytest.mark.parametrize("which", ["tiny", "vocab1100", "blank64", "blank255", "blank1050"])
def test_mixed_rows_in_one_launch(which, tiny_model, model_dir, request):
    """V = 40: three of the four waves hold no candidate; V = 1100: more than one logit per lane; blank64 / blank255 / blank1050: the
    blank logit in another wave than wave 0, in the last lane, past the first stride"""
    import april_asr_amd as A
    from april_asr_amd import synth_model as SM
    path = tiny_model["path"]
    if which == "vocab1100":
        path = str(model_dir / "tiny_vocab1100_so.april")
        SM.write_model(path, dict(SM.TINY_DIMS, vocab=1100))
    elif which in BM.MODELS:
        path = BM.model_info(which, request)["path"]
    gm = A.Model(path)
    assert (gm.dims.vocab, gm.dims.blank_id) == dict(tiny=(40, 0), vocab1100=(1100, 0), **BM.MODELS)[which]
    check_mixed_rows(gm)
    gm.close()


def check_mixed_rows(gm):
    """rows with, without and with default options in one launch of the OPT forms against search_options_ref and aprilx_run_decide
    (also what tests/device_optin_mutant_worker.py runs against every mutant of the OPT lines)"""
    V, blank = gm.dims.vocab, gm.dims.blank_id
    cls = R.token_classes(texts_of(gm))
    rng = np.random.default_rng(V)
    n = 16
    kinds = [None, (2200, 0.0), (300, 1.5), (700, -2.0)]
    custom = 0
    for step in range(6):
        rows = rng.normal(0.0, 2.0, (n, V)).astype(np.float32)
        rows[:, blank] += 2.5
        opts = [kinds[(i + step) % 4] for i in range(n)]
        toks = rng.integers(1, V, (n, 3))
        state = np.stack([[blank if rng.random() < 0.3 else toks[i, 0], toks[i, 1], -1 if rng.random() < 0.3 else toks[i, 2], 1000] for i in range(n)]).astype(np.int32)
        now = (1000 + rng.choice([0, 100, 299, 300, 699, 700, 2199, 2200, 5000], n)).astype(np.int32)
        rnd = step % 3
        ee = 1.0 if rnd == 0 else 0.0
        rec, st, _ = gm.run_decide_opts(rows, ee, now, rnd, state, opts)
        plain, pst = decide_plain(gm, rows, ee, now, rnd, state)
        for i, o in enumerate(opts):
            if o is None or o == (2200, 0.0):
                assert rec[i].tobytes() == plain[i].tobytes() and st[i].tobytes() == pst[i].tobytes(), (step, i, o)
                continue
            s = R.Search(cls, blank, (o[0], o[1], 0))
            s.set_state(state[i])
            idx, mx, bl = R.argmax_record(rows[i], blank)
            is_blank, _, changed = s.step(idx, mx, bl, ee, int(now[i]))
            assert int(rec["idx"][i]) == idx and bits(rec["max"][i]) == bits(mx) and bits(rec["blank"][i]) == bits(bl), (step, i)      # the RAW blank logit
            assert int(rec["flags"][i]) == (VALID | (BLANK if is_blank else 0) | (CTX if changed else 0)), (step, i, o)
            assert list(st[i]) == s.state(), (step, i, o)
            custom += rec[i].tobytes() != plain[i].tobytes() or st[i].tobytes() != pst[i].tobytes()
    assert custom > 0, "the rows with options of their own must decide differently somewhere"


# ---------------------------------------------------------------- 2. the hand-derived cases on the device
DEVICE_CASES = [c for c in G.CASES if c["device"]]


@pytest.mark.parametrize("case", DEVICE_CASES, ids=[c["name"] for c in DEVICE_CASES])
def test_device_matches_hand_derived(tiny, tiny_model, case):
    import april_asr_amd as A
    host = A.Model.load_host_only(tiny_model["path"])
    check_device_case(tiny, host, case, W.symbols(tiny_model["tokens"]))
    host.close()


def test_device_matches_hand_derived_with_the_blank_at_the_last_id(request):
    """every device case on blank39 in one test: the rows with and without options, the host state machine beside them"""
    import april_asr_amd as A
    info = BM.model_info("blank39", request)
    gm, host = A.Model(info["path"]), A.Model.load_host_only(info["path"])
    assert gm.dims.blank_id == 39
    for case in DEVICE_CASES:
        check_device_case(gm, host, case, W.symbols(info["tokens"]))
    host.close(); gm.close()


def check_device_case(gm, host, case, sym):
    """one hand-derived case on the device, beside a row without options and beside the host state machine (also what
    tests/device_optin_mutant_worker.py runs against every mutant of the OPT lines)"""
    V, blank = gm.dims.vocab, gm.dims.blank_id
    assert sym["<blk>"] == blank
    g = W.ProductGreedy(host, case["opts"])
    o = None if case["opts"] is None else (case["opts"][0], case["opts"][1])
    st = np.array([[blank, blank, -1, 0]] * 2, np.int32)
    for i, ((t, mx, bl, early, now), exp) in enumerate(zip(case["rounds"], case["expect"])):
        row = scripted_row(V, blank, sym[t], mx, bl)
        before = st.copy()
        # row 0: the case; row 1: the same inputs through a row without options, which must be aprilx_run_decide's
        rec, st, _ = gm.run_decide_opts(np.stack([row, row]), early, [now, now], 0 if early else 1, np.stack([before[0], before[0]]), [o, None])
        plain, pst = decide_plain(gm, row[None], early, [now], 0 if early else 1, before[:1])
        assert rec[1].tobytes() == plain[0].tobytes() and st[1].tobytes() == pst[0].tobytes(), (case["name"], i)
        want_flags = VALID | (BLANK if exp[0] else 0) | (CTX if exp[4] else 0)
        assert int(rec["idx"][0]) == sym[t] and bits(rec["max"][0]) == bits(mx) and bits(rec["blank"][0]) == bits(bl), (case["name"], i)
        assert int(rec["flags"][0]) == want_flags, (case["name"], i, int(rec["flags"][0]), want_flags)
        assert list(st[0]) == [sym[exp[1][0]], sym[exp[1][1]], -1 if exp[2] is None else sym[exp[2]], exp[3]], (case["name"], i, list(st[0]), exp)
        h_blank, h_ctx = g.step(sym[t], mx, bl, early, now)
        assert h_blank == exp[0] and list(h_ctx) == list(st[0][:2]), (case["name"], i)
    assert g.events == W.want_events(case, sym)
    g.close()


# ---------------------------------------------------------------- 3. with bias sets: back to the root at the session's own E
@pytest.mark.parametrize("strict", [False, True])
def test_bias_state_returns_to_the_root_at_E(tiny, strict):
    check_bias_state_returns_to_the_root_at_E(tiny, strict)


def check_bias_state_returns_to_the_root_at_E(gm, strict):
    texts, V, blank = texts_of(gm), gm.dims.vocab, gm.dims.blank_id
    words = [i for i, t in enumerate(texts) if t[:1] == b" " and i != blank]
    a, b = words[3], words[5]
    bias = gm.bias([(texts[a] + texts[b], 2.0)], strict=strict)
    tok, nxt, _ = bias.edges(0)
    s1 = int(nxt[list(tok).index(a)])
    assert s1 != 0
    row = np.full(V, -20.0, np.float32)
    row[blank] = 10.0                                              # every row resolves to blank
    #            options        gap   set   -> silence
    plan = [((700, 0.0), 699, True, False), ((700, 0.0), 700, True, True), ((700, 0.0), 2199, True, True),
            (None, 699, True, False), (None, 2199, True, False), (None, 2200, True, True),
            ((700, 0.0), 700, False, True), ((700, 1.0), 700, True, True)]
    n = len(plan)
    state = np.array([[blank, a, a, 1000]] * n, np.int32)
    now = np.array([1000 + p[1] for p in plan], np.int32)
    bs = np.array([s1 if p[2] else -1 for p in plan], np.int32)
    rec, st, bs2 = gm.run_decide_opts(np.stack([row] * n), 1.0, now, 0, state, [p[0] for p in plan], bias=bias, bias_state=bs)
    for i, (o, gap, has_set, silence) in enumerate(plan):
        assert int(rec["flags"][i]) == (VALID | BLANK), (i, int(rec["flags"][i]))
        assert int(bs2[i]) == ((0 if silence else s1) if has_set else -1), (i, plan[i], int(bs2[i]))
        assert list(st[i]) == [blank, a, -1 if silence else a, 1000], (i, list(st[i]))
    bias.close()


# ---------------------------------------------------------------- 4. live sessions
def pcm_of(i):
    return np.concatenate([speech_like_pcm(2.0, seed=40 + i, silence=(0.8, 1.5)), np.zeros(16000, np.int16), speech_like_pcm(1.0, seed=60 + i)])


OPTS = [(300, 1.5, 0), (300, -1.5, 0), (300, 1.5, 0), (300, -1.5, 0), None, None, None, None]


def run_group(gm, pcms, opts, feed=1600, trace=True, check_ctx=False, k=None):
    """len(pcms) sessions in lock step, `feed` samples at a time, then a flush: per session (events, traced logits, chunks, info log)"""
    import april_asr_amd as A
    n = len(pcms)
    evs = [[] for _ in range(n)]
    ss = []
    for i in range(n):
        o = opts[i]
        s = A.Session(gm, (lambda q: (lambda t, toks: evs[q].append((t, toks))))(i), raw_events=True, alternatives=k,
                      **({} if o is None else dict(endpoint_silence_ms=o[0], blank_penalty=o[1], max_utterance_ms=o[2])))
        assert s.search_options == (None if o is None else (o[0], float(np.float32(o[1])), o[2]))
        s.info_log = [] if k else None
        if trace:
            s.trace_logits(4000)
        ss.append(s)
    g = A.SessionGroup(ss)
    size = max(p.size for p in pcms)
    for off in range(0, size, feed):
        g.feed([p[off:off + feed] for p in pcms])
        if check_ctx:
            for s in ss:
                h, d = s.contexts()
                assert list(h) == list(d[:2]), "context: host %s, device %s" % (list(h), list(d))
    g.flush()
    out = []
    for i, s in enumerate(ss):
        assert s.search_options == (None if opts[i] is None else (opts[i][0], float(np.float32(opts[i][1])), opts[i][2])), "the options must survive the flush"
        out.append((evs[i], s.traced_logits().copy() if trace else None, s.chunks(), s.info_log))
        s.close()
    return out


def as_text_events(events, texts):
    return [(t, [(texts[i], lp, fl, ms) for (i, lp, fl, ms) in toks]) for t, toks in events]


def same_events(a, b):
    assert [(t, len(k)) for t, k in a] == [(t, len(k)) for t, k in b]
    for (_, k0), (_, k1) in zip(a, b):
        for x, y in zip(k0, k1):
            assert x[0] == y[0] and x[2:] == y[2:], (x, y)
            assert bits(x[1]) == bits(y[1]), (x, y)


@pytest.fixture(scope="module")
def baseline(tiny_model):
    """the eight streams on an engine where nobody ever opted in"""
    import april_asr_amd as A
    gm = A.Model(tiny_model["path"])
    pcms = [pcm_of(i) for i in range(8)]
    out = run_group(gm, pcms, [None] * 8)
    assert gm.stats().replay_mismatch == 0
    gm.close()
    return pcms, out


def test_live_sessions(tiny_model, baseline):
    import april_asr_amd as A
    pcms, base = baseline
    gm = A.Model(tiny_model["path"])
    texts, blank = texts_of(gm), gm.dims.blank_id
    cls = R.token_classes(texts)
    got = run_group(gm, pcms, OPTS, check_ctx=True)                 # 100 ms feeds: the feed wavefront
    st = gm.stats()
    assert st.replay_mismatch == 0 and st.wave_steps > 0
    differs = 0
    for i in range(8):
        ev, lg, chunks, _ = got[i]
        if OPTS[i] is None:
            assert lg.tobytes() == base[i][1].tobytes() and ev == base[i][0], "a session without options differs from the engine where nobody opted in (%d)" % i
            continue
        want, _ = R.replay(cls, blank, OPTS[i], lg, chunks)
        same_events(ev, as_text_events(want, texts))
        differs += ev != base[i][0]
        print("session %d %s: %d events (%d FINAL), without options %d (%d FINAL)" % (i, OPTS[i], len(ev), sum(t == 2 for t, _ in ev), len(base[i][0]), sum(t == 2 for t, _ in base[i][0])))
    assert differs > 0, "the options must matter on these streams"
    # one long feed: the layer-major path; the same stream, the same options -> the same events, and again the reference's
    lm0 = gm.stats().lm_steps
    ev, lg, chunks, _ = run_group(gm, [pcms[0]], [OPTS[0]], feed=pcms[0].size, check_ctx=True)[0]
    assert gm.stats().lm_steps > lm0
    same_events(ev, as_text_events(R.replay(cls, blank, OPTS[0], lg, chunks)[0], texts))
    same_events(ev, got[0][0])
    # untraced (captured graphs): the same events
    ev_g = run_group(gm, pcms[:2], OPTS[:2], trace=False)
    same_events(ev_g[0][0], got[0][0]); same_events(ev_g[1][0], got[1][0])
    assert gm.stats().replay_mismatch == 0
    gm.close()


def info_bytes(info, eval_index):
    b = _copy_info(info)
    b.eval_index = eval_index
    return bytes(b)


def _copy_info(info):
    from april_asr_amd import _ffi
    return _ffi.AprilxTokenInfo.from_buffer_copy(bytes(info))


def test_confidences_keep_the_raw_values(tiny_model, baseline):
    import april_asr_amd as A
    from april_asr_amd import _ffi
    pcms, _ = baseline
    gm = A.Model(tiny_model["path"])
    blank = gm.dims.blank_id
    plain = run_group(gm, pcms[:1], [None], k=4)[0]
    dflt = run_group(gm, pcms[:1], [(2200, 0.0, 0)], k=4)[0]
    assert plain[0] == dflt[0] and plain[3] == dflt[3] and len(plain[3]) > 0, "default options change the side records"
    ev, lg, chunks, log = run_group(gm, pcms[:1], [(300, 1.5, 0)], k=4)[0]
    n_tok = 0
    for (t, toks), (t2, infos) in zip(ev, log):
        assert t == t2 and len(toks) == len(infos)
        for (text, logprob, flags, ms), raw in zip(toks, infos):
            info = _ffi.AprilxTokenInfo.from_buffer_copy(raw)
            row = lg[int(info.eval_index)]
            idx, mx, bl = R.argmax_record(row, blank)
            assert int(info.alt_id[0]) == idx and bits(info.alt_logit[0]) == bits(mx)
            assert bits(info.blank_logprob) == bits(np.float32(bl - np.float32(info.lse))), "the penalty leaked into the side record"
            assert bits(np.float32(logprob)) in (bits(mx), bits(np.float32(mx - np.float32(8.0)))), "AprilToken.logprob is the raw logit"
            n_tok += 1
    assert n_tok > 0 and gm.stats().replay_mismatch == 0
    # every side record of the session with p = 1.5, byte for byte, against the same row WITHOUT options through the same device code
    # (the sessions are closed: aprilx_run_confidence uses the first slots itself)
    used = sorted({int(_ffi.AprilxTokenInfo.from_buffer_copy(raw).eval_index) for _, infos in log for raw in infos})
    plain_rec = {}
    for o in range(0, len(used), 64):
        part = used[o:o + 64]
        for e, rec in zip(part, gm.run_confidence(lg[part], 4)):
            plain_rec[e] = info_bytes(rec, e)
    for _, infos in log:
        for raw in infos:
            e = int(_ffi.AprilxTokenInfo.from_buffer_copy(raw).eval_index)
            assert bytes(raw) == plain_rec[e], "evaluation %d: the side record of a session with options differs from the row's without" % e
    gm.close()


def test_bias_set_confidences_and_options_together(tiny_model, baseline):
    """decide_conf_bias_opt_kernel in a live session: a boosting set, K = 4 and E = 300 / p = 1.5 at once.  The session is replayed from its
    raw traced logits -- bias_ref.py adds the bonuses, search_options_ref.py decides --; every side record equals, byte for byte, the one
    aprilx_run_confidence_biased gives for the same row and trie state without options."""
    import april_asr_amd as A
    from april_asr_amd import _ffi
    import bias_ref as BR
    import bias_worker as BW
    pcms, _ = baseline
    gm = A.Model(tiny_model["path"])
    texts, blank = texts_of(gm), gm.dims.blank_id
    cls = R.token_classes(texts)
    phrases = BW.session_phrases(texts, blank, np.random.default_rng(3))
    ref, bias = BR.BiasRef(texts, blank, phrases), gm.bias(phrases)
    opts = (300, 1.5, 0)
    runs = {}
    for o in (None, (2200, 0.0, 0), opts):
        ev = []
        s = A.Session(gm, lambda t, toks: ev.append((t, toks)), raw_events=True, bias=bias, alternatives=4,
                      **({} if o is None else dict(endpoint_silence_ms=o[0], blank_penalty=o[1])))
        s.info_log = []
        s.trace_logits(4000)
        for off in range(0, pcms[0].size, 1600):
            s.feed_pcm16(pcms[0][off:off + 1600])
            h, d = s.bias_state()
            assert h == d, "trie state: host %d, device %d" % (h, d)
            hc, dc = s.contexts()
            assert list(hc) == list(dc[:2])
        s.flush()
        runs[o] = (ev, s.traced_logits().copy(), s.chunks(), s.info_log)
        s.close()
    assert runs[None][0] == runs[(2200, 0.0, 0)][0] and runs[None][3] == runs[(2200, 0.0, 0)][3] and len(runs[None][3]) > 0, "default options change a biased session"
    ev, lg, chunks, log = runs[opts]
    # the reference: v' = v + bonus(state), the decision with options on v', the trie state moved with it
    g, srch = R.Greedy(cls, blank, opts), R.Search(cls, blank, opts)
    st, states, row = 0, [], 0
    for c in range(1, chunks + 1):
        for r in range(3):
            states.append(st)
            idx, mx, bl = R.argmax_record(ref.biased(lg[row], st), blank)
            ee = 1.0 if r == 0 else 0.0
            is_blank = g.step(idx, mx, bl, ee, c * 40)
            _, silence, _ = srch.step(idx, mx, bl, ee, c * 40)
            st = ref.next(st, idx) if not is_blank else (0 if silence else st)
            row += 1
            if is_blank:
                break
    assert row == len(lg)
    g.finish()
    same_events(ev, as_text_events(g.events, texts))
    assert sum(1 for x in states if x) > 0, "the run must reach states inside phrases"
    used = sorted({int(_ffi.AprilxTokenInfo.from_buffer_copy(raw).eval_index) for _, infos in log for raw in infos})
    want = {}
    for o in range(0, len(used), 64):
        part = used[o:o + 64]
        for e, rec in zip(part, gm.run_confidence_biased(lg[part], 4, bias, [states[e] for e in part])):
            want[e] = info_bytes(rec, e)
    assert len(used) > 0
    for _, infos in log:
        for raw in infos:
            e = int(_ffi.AprilxTokenInfo.from_buffer_copy(raw).eval_index)
            assert bytes(raw) == want[e], "evaluation %d: side record differs from the same row and state without options" % e
    assert gm.stats().replay_mismatch == 0
    bias.close(); gm.close()


# ---------------------------------------------------------------- 5. life cycle
def test_life_cycle(tiny_model, baseline):
    import april_asr_amd as A
    from april_asr_amd import _ffi
    pcms, base = baseline
    gm = A.Model(tiny_model["path"])
    L = gm._L
    s = A.Session(gm, lambda t, toks: None, raw_events=True)
    assert s.search_options is None
    o = _ffi.AprilxSearchOptions()
    assert L.aprilx_session_search_options(s._handle, C.byref(o)) == 0 and (o.size, o.endpoint_silence_ms, o.max_utterance_ms, o.blank_penalty) == (16, 2200, 0, 0.0)
    s.set_search_options(700, 1.0, 5000)
    assert s.search_options == (700, 1.0, 5000)
    for E, p, U, dsize in G.REFUSED:
        assert L.aprilx_session_set_search_options(s._handle, C.byref(W.make_options((E, p, U), dsize))) == -1, (E, p, U, dsize)
        assert s.search_options == (700, 1.0, 5000)
    for acc in G.ACCEPTED:
        s.set_search_options(*[acc[0], acc[1], acc[2]])
        assert s.search_options == (acc[0], acc[1], acc[2])
    s.set_search_options(700, 1.0, 5000)
    s.feed_pcm16(pcms[0][:1600])                                    # audio fed since the last flush: refused, nothing changes
    with pytest.raises(ValueError):
        s.set_search_options(300)
    with pytest.raises(ValueError):
        s.set_search_options()
    assert s.search_options == (700, 1.0, 5000)
    s.flush()
    assert s.search_options == (700, 1.0, 5000)                      # survives the flush, and may change again
    s.set_search_options(300)
    assert s.search_options == (300, 0.0, 0)
    s.set_search_options()
    assert s.search_options is None
    s.set_search_options(300, 1.5)
    s.close()
    # A freed slot is handed out again once a flight has reset it.  Four sessions run with E = 300, p = 1.5 and are freed; one more session
    # runs a feed and a flush (the flights that return those four slots to the free list, last freed first out); the next four sessions
    # then own exactly those slots.  They start without options: their streams are those of the engine where nobody opted in (a slot that
    # kept E = 300 / p = 1.5 on the device would decide differently from the host's replay: other events and replay_mismatch > 0).
    opted = run_group(gm, pcms[:4], [(300, 1.5, 0)] * 4)
    assert any(opted[i][0] != base[i][0] for i in range(4)), "the options must matter on these streams"
    helper = A.Session(gm, lambda t, toks: None, raw_events=True)
    helper.feed_pcm16(pcms[5][:3200])
    helper.flush()
    got = run_group(gm, pcms[:4], [None] * 4)
    helper.close()
    for i in range(4):
        assert got[i][0] == base[i][0] and got[i][1].tobytes() == base[i][1].tobytes(), i
    assert gm.stats().replay_mismatch == 0
    gm.close()


def test_first_opt_in_with_captured_graphs(tiny_model, baseline):
    """sessions that run on captured graphs keep their transcripts when another session's first opt-in drops those graphs mid-stream"""
    import april_asr_amd as A
    pcms, base = baseline
    gm = A.Model(tiny_model["path"])
    evs = [[] for _ in range(5)]
    ss = [A.Session(gm, (lambda q: (lambda t, toks: evs[q].append((t, toks))))(i), raw_events=True) for i in range(4)]
    g = A.SessionGroup(ss)
    half = (pcms[0].size // 3200) * 1600
    for off in range(0, half, 1600):
        g.feed([p[off:off + 1600] for p in pcms[:4]])
    late = A.Session(gm, lambda t, toks: evs[4].append((t, toks)), raw_events=True, endpoint_silence_ms=300, blank_penalty=1.5)      # the engine's first opt-in
    g5 = A.SessionGroup(ss + [late])
    for off in range(half, pcms[0].size, 1600):
        g5.feed([p[off:off + 1600] for p in pcms[:4]] + [pcms[4][off - half:off - half + 1600]])
    g5.flush()
    for i in range(4):
        assert evs[i] == base[i][0], "session %d changed when the engine's first opt-in arrived" % i
    assert len(evs[4]) > 0 and gm.stats().replay_mismatch == 0
    for s in ss + [late]:
        s.close()
    gm.close()


def test_three_first_opt_ins_in_one_flight_with_captured_graphs(tiny_model, baseline):
    """the engine's first bias set, first K > 0 and first search options arrive together, with one session, while four plain sessions run
    on captured graphs: all three tables are applied in the same begin_flight.  The plain sessions keep their transcripts; the late
    session's events and side records are those of the same session alone on a fresh model where the three were set before any audio."""
    import april_asr_amd as A
    import bias_worker as BW
    pcms, base = baseline
    half = (pcms[0].size // 3200) * 1600
    late_pcm = pcms[4][:pcms[0].size - half]

    def late_session(gm, ev):
        texts = texts_of(gm)
        bias = gm.bias(BW.session_phrases(texts, gm.dims.blank_id, np.random.default_rng(3)))
        s = A.Session(gm, lambda t, toks: ev.append((t, toks)), raw_events=True, bias=bias, alternatives=4, endpoint_silence_ms=300, blank_penalty=1.5)
        s.info_log = []
        return s, bias

    def states_agree(s):
        h, d = s.bias_state()
        assert h == d, "trie state: host %d, device %d" % (h, d)

    gm = A.Model(tiny_model["path"])
    evs = [[] for _ in range(5)]
    ss = [A.Session(gm, (lambda q: (lambda t, toks: evs[q].append((t, toks))))(i), raw_events=True) for i in range(4)]
    g = A.SessionGroup(ss)
    for off in range(0, half, 1600):
        g.feed([p[off:off + 1600] for p in pcms[:4]])
    late, bias = late_session(gm, evs[4])                          # the engine's first opt-in of all three kinds
    g5 = A.SessionGroup(ss + [late])
    for off in range(half, pcms[0].size, 1600):
        g5.feed([p[off:off + 1600] for p in pcms[:4]] + [late_pcm[off - half:off - half + 1600]])
        states_agree(late)
    g5.flush()
    for i in range(4):
        assert evs[i] == base[i][0], "session %d changed when the engine's first opt-ins arrived" % i
    assert gm.stats().replay_mismatch == 0
    log = late.info_log
    for s in ss + [late]:
        s.close()
    bias.close(); gm.close()

    gm = A.Model(tiny_model["path"])
    ev1 = []
    alone, bias = late_session(gm, ev1)
    for off in range(0, late_pcm.size, 1600):
        alone.feed_pcm16(late_pcm[off:off + 1600])
        states_agree(alone)
    alone.flush()
    assert len(evs[4]) > 0 and evs[4] == ev1, "the late session differs from the same session alone"
    assert [(t, [bytes(r) for r in infos]) for t, infos in log] == [(t, [bytes(r) for r in infos]) for t, infos in alone.info_log] and len(log) > 0
    assert gm.stats().replay_mismatch == 0
    alone.close(); bias.close(); gm.close()
