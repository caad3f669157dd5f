"""Phrase boosting inside the device search (aprilx_session_set_bias).

The statement of the contract is tests/bias_ref.py (checked against the host-side builder by tests/test_bias_cpu.py).  Here: the
decision kernel's biased form against it bit for bit on given rows, whole sessions reproduced from their raw traced logits, the
effect on a transcript, the invariances (batch, neighbours, schedule, pipelining, zero boosts), confidences on v', the life cycle.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bias_ref as R
import bias_worker as W
import blank_models as BM
import confidence_ref as CR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALID, BLANK = 1, 2


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def load(which, request, model_dir):
    import april_asr_amd as A
    from april_asr_amd import synth_model as SM
    if which == "vocab1100":
        path = str(model_dir / "tiny_vocab1100.april")
        SM.write_model(path, dict(SM.TINY_DIMS, vocab=1100))
    else:
        path = BM.model_info(which, request)["path"]
    gm = A.Model(path)
    assert gm.dims.vocab == dict(tiny=40, medium=131, v0=500, vocab1100=1100, **{k: v[0] for k, v in BM.MODELS.items()})[which]
    assert gm.dims.blank_id == BM.MODELS.get(which, (0, 0))[1]
    return gm


def decide_plain(gm, lg, ee, now, rnd, state):
    st = np.ascontiguousarray(state, np.int32).copy()
    n = st.shape[0]
    rec = np.zeros(n, np.dtype([("idx", np.int32), ("max", np.float32), ("blank", np.float32), ("flags", np.uint32)]))
    nowa = np.ascontiguousarray(now, np.int32)
    lg = np.ascontiguousarray(lg, np.float32)
    assert gm._L.aprilx_run_decide(gm._handle, n, 0, lg.ctypes.data, C.c_float(ee), nowa.ctypes.data, rnd, st.ctypes.data, rec.ctypes.data) == 0
    return rec, st


def check_rows(gm, ref, bias, searches, rows, ee, now, rnd, what):
    """one launch: row i of `rows` for searches[i] (a R.Search; .ref None = a row without a set)"""
    n = len(searches)
    st = np.array([s.state() for s in searches], np.int32)
    bs = np.array([s.s if s.ref is not None else -1 for s in searches], np.int32)
    rec, st2, bs2 = gm.run_decide_biased(rows, ee, now, rnd, st, bias, bs)
    for i, s in enumerate(searches):
        idx, mx, bl, is_blank = s.step(rows[i], ee, int(now[i]))
        assert rec["flags"][i] & VALID
        assert int(rec["idx"][i]) == idx, (what, i, int(rec["idx"][i]), idx)
        assert bits(rec["max"][i]) == bits(mx) and bits(rec["blank"][i]) == bits(bl), (what, i)
        assert bool(rec["flags"][i] & BLANK) == is_blank, (what, i)
        assert list(st2[i]) == s.state(), (what, i)
        assert int(bs2[i]) == (s.s if s.ref is not None else -1), (what, i, int(bs2[i]), s.s)
    return rec, st2


# ---------------------------------------------------------------- 1. the decision kernel on given rows
@pytest.mark.parametrize("which", ["tiny", "medium", "v0", "vocab1100", "blank64", "blank255", "blank1050"])
def test_scripted_rounds(which, request, model_dir):
    gm = load(which, request, model_dir)
    check_scripted_rounds(gm)
    gm.close()


def check_scripted_rounds(gm, trials=2):
    """the biased decision kernel on hand-made rows and on random rounds against bias_ref, bit for bit (also what
    tests/device_optin_mutant_worker.py runs against every mutant of the bias lines)"""
    texts, blank, V = W.model_texts(gm), gm.dims.blank_id, gm.dims.vocab
    cls = R.token_classes(texts)
    words = [i for i, t in enumerate(texts) if t[:1] == b" " and i != blank]
    # ---- hand-made rows: one phrase of two word tokens a, b with boost 2; c is an unboosted token with a lower id than a where possible
    a, b = words[3], words[5]
    lo = [i for i in range(1, a) if i != blank and not (cls[i] & 6) and texts[a].find(texts[i]) != 0]
    c = lo[0] if lo else [i for i in words if i not in (a, b)][0]
    phrases = [(texts[a] + texts[b], 2.0)]
    ref, bias = R.BiasRef(texts, blank, phrases), gm.bias(phrases)
    assert a in ref.eff[0] and c not in ref.eff[0]
    two = np.float32(2.0)

    def row(**kv):
        r = np.full(V, -20.0, np.float32)
        r[blank] = -10.0
        for k, v in kv.items():
            r[int(k[1:])] = v
        return r
    cases = [
        ("runner-up promoted by its bonus", row(**{"t%d" % a: 3.0, "t%d" % c: 4.5}), 0.0, a),
        ("bonus too small to change the winner", row(**{"t%d" % a: 3.0, "t%d" % c: 5.5}), 0.0, c),
        ("tie between a boosted and an unboosted token: the lower id", row(**{"t%d" % a: 3.0, "t%d" % c: 5.0}), 0.0, min(a, c)),
        ("blank loses by the bonus", row(**{"t%d" % a: 3.0, "t%d" % blank: 4.0}), 0.0, a),
        ("blank wins although the token is boosted", row(**{"t%d" % a: 3.0, "t%d" % blank: 5.5}), 0.0, a),
        ("blank wins by the early-emit margin exactly at the bonus", row(**{"t%d" % a: 3.0, "t%d" % blank: 6.0}), 1.0, a),
    ]
    for what, r, ee, want_idx in cases:
        s_b, s_0 = R.Search(cls, blank, ref), R.Search(cls, blank, None)
        s_b.ctx = [blank, c]; s_0.ctx = [blank, c]                       # (not a cleared context)
        rec, _ = check_rows(gm, ref, bias, [s_b, s_0], np.stack([r, r]), ee, np.array([40, 40], np.int32), 0, what)
        assert int(rec["idx"][0]) == want_idx, what
        plain, _ = decide_plain(gm, r[None], ee, [40], 0, [[blank, c, -1, 0]])
        assert rec[1].tobytes() == plain[0].tobytes(), "a row without a set differs from aprilx_run_decide: " + what
    assert bits(np.float32(3.0) + two) == bits(np.float32(5.0))
    # ties between ids that ONE lane of bias_scan compares (n, n + 256, ...): the lower id wins only because ids ascend within a lane and
    # the comparison is strict.  d: unboosted ids in a's lane; x: a lane without a boosted token
    lane_a = [n for n in range(a + 256, V, 256) if n != blank and n not in ref.eff[0]]
    x = next(n for n in range(20, 256) if all(m != blank and m not in ref.eff[0] for m in range(n, V, 256)))
    lane_x = list(range(x + 256, V, 256))
    ties = []
    for d in lane_a:
        ties.append(("a tie that exists only after the bonus, %d apart: the boosted lower id" % (d - a), row(**{"t%d" % a: 3.0, "t%d" % d: 5.0}), a))
        ties.append(("the boosted token behind by less than its bonus: the higher id", row(**{"t%d" % a: 2.75, "t%d" % d: 5.0}), d))
    for d in lane_x:
        ties.append(("a raw tie %d apart in a row with a set" % (d - x), row(**{"t%d" % x: 5.0, "t%d" % d: 5.0}), x))
    if len(lane_x) >= 2:
        ties.append(("a raw tie of three in one lane", row(**{"t%d" % n: 5.0 for n in [x] + lane_x[:2]}), x))
        ties.append(("a raw tie of the lane's second and third id", row(**{"t%d" % n: 5.0 for n in lane_x[:2]}), lane_x[0]))
    assert (len(ties) >= 3) == (V >= 500)
    for what, r, want_idx in ties:
        s_b, s_0 = R.Search(cls, blank, ref), R.Search(cls, blank, None)
        s_b.ctx = [blank, c]; s_0.ctx = [blank, c]
        rec, _ = check_rows(gm, ref, bias, [s_b, s_0], np.stack([r, r]), 0.0, np.array([40, 40], np.int32), 0, what)
        assert int(rec["idx"][0]) == want_idx and not (rec["flags"][0] & BLANK), (what, int(rec["idx"][0]), want_idx)
        plain, _ = decide_plain(gm, r[None], 0.0, [40], 0, [[blank, c, -1, 0]])
        assert rec[1].tobytes() == plain[0].tobytes(), "a row without a set differs from aprilx_run_decide: " + what
    # punctuation override reached through the bonus: a phrase that ends in the comma token; 2.0 + 2 > 5.0 - 3.5 but 2.0 is not
    comma = [i for i, t in enumerate(texts) if t == b","]
    if comma:
        p2 = [(texts[a] + b",", 2.0)]
        ref2, bias2 = R.BiasRef(texts, blank, p2), gm.bias(p2)
        s_b, s_0 = R.Search(cls, blank, ref2), R.Search(cls, blank, None)
        for s in (s_b, s_0):
            s.ctx = [blank, a]; s.last_tok = a
        s_b.s = ref2.next(0, a)
        assert comma[0] in ref2.eff[s_b.s]
        r = row(**{"t%d" % comma[0]: 0.0, "t%d" % blank: 5.0})
        rec, _ = check_rows(gm, ref2, bias2, [s_b, s_0], np.stack([r, r]), 0.0, np.array([80, 80], np.int32), 1, "punctuation override")
        assert not (rec["flags"][0] & BLANK) and (rec["flags"][1] & BLANK), "the override must be reached through the bonus only"
        bias2.close()
    # negative boost: the token loses although its logit is the highest
    p3 = [(texts[a], -3.0)]
    ref3, bias3 = R.BiasRef(texts, blank, p3), gm.bias(p3)
    s_b = R.Search(cls, blank, ref3)
    rec, _ = check_rows(gm, ref3, bias3, [s_b], row(**{"t%d" % a: 5.0, "t%d" % c: 3.0})[None], 0.0, np.array([40], np.int32), 0, "negative boost")
    assert int(rec["idx"][0]) == c
    # end-of-flush reset (op 1): states back to the root
    _, st, bs = gm.run_decide_biased(np.zeros((2, V), np.float32), 0.0, [0, 0], 0, [[a, b, a, 7], [blank, blank, -1, 0]], bias, [ref.next(0, a), -1], op=1)
    assert list(bs) == [0, -1] and list(st[0]) == [blank, blank, -1, 7]
    bias.close(); bias3.close()

    # ---- 2 x 1500 random rounds with random sets: 50 rows per launch (every fifth without a set), 30 launches in sequence
    for trial in range(trials):
        rng = np.random.default_rng(1000 * trial + V)
        phrases = W.session_phrases(texts, blank, rng, n=5 + 25 * trial)
        phrases[0] = (phrases[0][0], -2.0); phrases[1] = (phrases[1][0], 0.0)
        ref, bias = R.BiasRef(texts, blank, phrases), gm.bias(phrases)
        searches = [R.Search(cls, blank, ref if i % 5 else None) for i in range(50)]
        now = np.zeros(50, np.int32)
        moved = 0
        for step in range(30):
            rows = rng.normal(0.0, 2.0, (50, V)).astype(np.float32)
            rows[:, blank] += 2.0
            for i, s in enumerate(searches):                        # pull the search along the phrases, so that deep states are reached
                e = sorted(ref.eff[s.s])
                if e and rng.random() < 0.6:
                    rows[i, int(rng.choice(e))] += np.float32(4.0)
            now += rng.choice([40, 40, 80, 2300], 50).astype(np.int32)
            rnd = int(rng.integers(0, 3))
            plain_rows = [i for i, s in enumerate(searches) if s.ref is None]
            st_before = np.array([searches[i].state() for i in plain_rows], np.int32)
            rec, _ = check_rows(gm, ref, bias, searches, rows, 1.0 if rnd == 0 else 0.0, now, rnd, "trial %d step %d" % (trial, step))
            plain, _ = decide_plain(gm, rows[plain_rows], 1.0 if rnd == 0 else 0.0, now[plain_rows], rnd, st_before)
            assert rec[plain_rows].tobytes() == plain.tobytes(), "rows without a set differ from aprilx_run_decide"
            moved += sum(1 for s in searches if s.s)
        assert moved > 100, "the random rounds must reach states inside phrases"
        bias.close()


# ---------------------------------------------------------------- 2. whole sessions from their raw traced logits
@pytest.mark.parametrize("which", ["tiny", "v0"])
def test_whole_sessions(which, request, model_dir):
    gm = load(which, request, model_dir)
    n_tok, moved, differs = W.whole_session(gm)
    print("%s (V = %d, %d layers): %d tokens delivered, %d evaluations started inside a phrase, transcript differs from the unbiased one: %s" % (which, gm.dims.vocab, gm.dims.n_layers, n_tok, moved, differs))
    assert n_tok > 0 and moved > 0, "the run must reach states inside phrases"
    assert differs, "the set must change this transcript"
    gm.close()


def test_whole_session_fp16_engine(tiny_model):
    env = dict(os.environ, APRIL_PRECISION="f16", APRIL_LOG_LEVEL="NONE")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bias_worker.py"), tiny_model["path"]], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0 and "ok precision=1" in out, out[-2000:]


# ---------------------------------------------------------------- 3. the effect, end to end
def three_token_phrase(texts, blank):
    """three word tokens; where the vocabulary has them, three whose concatenation only they can walk (no other token is a prefix
    anywhere along the phrase)"""
    import itertools
    cls = R.token_classes(texts)
    words = [i for i, t in enumerate(texts) if t[:1] == b" " and len(t) >= 3 and i != blank and not (cls[i] & 16)]
    for ids in itertools.permutations(words[:12], 3):
        ref = R.BiasRef(texts, blank, [(b"".join(texts[i] for i in ids), 1.0)])
        if sum(len(e) for e in ref.eff) == ref.S + 2 and len(ref.eff[0]) == 1:
            return list(ids)
    return words[2:5]


@pytest.mark.parametrize("which", ["tiny", "v0"])
def test_effect_on_the_transcript(which, request, model_dir):
    gm = load(which, request, model_dir)
    texts, blank = W.model_texts(gm), gm.dims.blank_id
    ids = three_token_phrase(texts, blank)
    phrase = b"".join(texts[i] for i in ids)
    pcm = W.test_pcm()
    ev0, lg0, chunks0, _ = W.run(gm, pcm, 1600, trace=True)
    boost = min(100.0, 2.0 * float(np.ceil(lg0.max() - lg0.min())))   # larger than the whole logit spread of the unbiased run, with room
    assert boost <= 100.0
    phrases = [(phrase, boost)]
    ref, bias = R.BiasRef(texts, blank, phrases), gm.bias(phrases)
    ev, lg, chunks, _ = W.run(gm, pcm, 1600, bias=bias, trace=True, check_state=True)
    want, _, _ = W.replay(gm, texts, ref, lg, chunks)
    W.same_events(ev, want)
    finals = b"".join(t[0] for typ, toks in ev if typ == 2 for t in toks)
    finals0 = b"".join(t[0] for typ, toks in ev0 if typ == 2 for t in toks)
    # every evaluation now has a boosted token that beats the blank: the transcript is made of the phrase's pieces and nothing else
    pieces = {texts[n] for e in ref.eff for n in e}
    assert finals != finals0, (phrase, finals[:200], finals0[:200])
    assert {t[0] for typ, toks in ev if typ == 2 for t in toks} <= pieces, "a token without an edge beat a bonus larger than the logit spread"
    assert sum(len(toks) for typ, toks in ev if typ == 2) > sum(len(toks) for typ, toks in ev0 if typ == 2)
    bias.close(); gm.close()


# ---------------------------------------------------------------- 4. invariances
def test_alone_equals_among_255_unbiased(v0_model):
    import april_asr_amd as A
    from oracle import orc_py as O
    gm = A.Model(v0_model["path"])
    texts, blank = W.model_texts(gm), gm.dims.blank_id
    pcm = W.test_pcm(2.0)[:16000 * 6]
    n = 256
    pcms = [pcm] + [O.lcg_pcm16_fast(pcm.size, seed=700 + i) for i in range(1, n)]

    def many(bias0):
        evs = [[] for _ in range(n)]
        ss = [A.Session(gm, (lambda q: (lambda t, toks: evs[q].append((t, toks))))(i), raw_events=True, bias=bias0 if i == 0 else None) for i in range(n)]
        g = A.SessionGroup(ss)
        for o in range(0, pcm.size, 1600):
            g.feed([p[o:o + 1600] for p in pcms])
        assert ss[0].bias_state()[0] == ss[0].bias_state()[1]
        g.flush()
        for s in ss:
            s.close()
        return evs
    before = many(None)                                               # no biased session has ever been on this engine
    bias = gm.bias([(p, 8.0) for p, _ in W.session_phrases(texts, blank, np.random.default_rng(3))])
    among = many(bias)
    alone = W.run(gm, pcm, 1600, bias=bias)[0]
    assert among[0] == alone, "a biased session stepped alone differs from the same session among 255 unbiased ones"
    assert among[1:] == before[1:], "unbiased neighbours changed when a biased session joined the engine"
    assert among[0] != before[0], "the set must matter in this run"
    assert W.run(gm, pcm, 1600)[0] == before[0], "an unbiased session after the opt-in differs from before"
    assert gm.stats().replay_mismatch == 0
    bias.close(); gm.close()


def test_schedules_pipelining_and_zero_boosts(v0_model):
    import april_asr_amd as A
    gm = A.Model(v0_model["path"])
    texts, blank = W.model_texts(gm), gm.dims.blank_id
    phrases = W.session_phrases(texts, blank, np.random.default_rng(3))
    bias = gm.bias(phrases)
    pcm = W.test_pcm()
    ev = W.run(gm, pcm, 1600, bias=bias)[0]
    assert ev == W.run(gm, pcm, pcm.size, bias=bias)[0], "streaming differs from one long feed (layer-major / offline wavefront)"
    assert ev == W.run(gm, pcm, 16000, bias=bias)[0], "100 ms feeds differ from 1 s feeds (feed wavefront / layer-major)"
    assert ev == W.run(gm, pcm, 1600, bias=bias, mode="pipelined")[0], "lock-step differs from pipelined depth 2"
    zero = gm.bias([(p, 0.0) for p, _ in phrases])
    ev0 = W.run(gm, pcm, 1600)[0]
    assert ev0 == W.run(gm, pcm, 1600, bias=zero, check_state=True)[0], "a set with all boosts 0 changes the callbacks"     # (values, ==: -0.0 + 0.0)
    assert ev != ev0
    assert gm.stats().replay_mismatch == 0
    zero.close(); bias.close(); gm.close()


# ---------------------------------------------------------------- 5. with confidences on
def test_confidences_are_computed_on_the_biased_logits(v0_model):
    import april_asr_amd as A
    from april_asr_amd import _ffi
    gm = A.Model(v0_model["path"])
    texts, blank = W.model_texts(gm), gm.dims.blank_id
    phrases = W.session_phrases(texts, blank, np.random.default_rng(3))
    ref, bias = R.BiasRef(texts, blank, phrases), gm.bias(phrases)
    pcm = W.test_pcm()
    ev, lg, chunks, log = W.run(gm, pcm, 1600, bias=bias, trace=True, k=4, check_state=True)
    want, vps, states = W.replay(gm, texts, ref, lg, chunks)
    W.same_events(ev, want)
    n_tok = n_boosted = 0
    worst = 0.0
    for (t, toks), (t2, infos) in zip(ev, log):
        assert t == t2 and len(toks) == len(infos)
        for (text, logprob, flags, time_ms), raw in zip(toks, infos):
            info = _ffi.AprilxTokenInfo.from_buffer_copy(raw)
            vp = vps[int(info.eval_index)]
            worst = max(worst, CR.check_info(info, vp, blank, 4, "evaluation %d" % info.eval_index))     # lse against float64 on v', section 12's bound
            idx, mx, _ = R.argmax_record(vp, blank)
            assert int(info.alt_id[0]) == idx and bits(info.alt_logit[0]) == bits(mx)
            lp = np.float32(logprob)
            assert bits(lp) == bits(mx) or bits(lp) == bits(np.float32(mx - np.float32(8.0)))
            n_boosted += bits(vp[idx]) != bits(lg[int(info.eval_index)][idx])
            n_tok += 1
    print("%d tokens, %d of them with a bonus in their logit; worst lse error %.3f of the bound" % (n_tok, n_boosted, worst))
    assert n_tok > 0 and n_boosted > 0
    assert W.run(gm, pcm, 1600, bias=bias, k=4)[0] == ev              # untraced: decide_conf_bias_kernel under graph replay
    assert W.run(gm, pcm, 1600, bias=bias)[0] == ev                    # the confidences change no decision of a biased session either
    bias.close(); gm.close()


# ---------------------------------------------------------------- 6. life cycle
def test_life_cycle(tiny_model):
    import april_asr_amd as A
    gm = A.Model(tiny_model["path"])
    texts, blank = W.model_texts(gm), gm.dims.blank_id
    rng = np.random.default_rng(11)
    b1 = gm.bias(W.session_phrases(texts, blank, rng))
    b2 = gm.bias(W.session_phrases(texts, blank, rng))
    pcm = W.test_pcm(2.0)
    ev0, ev1, ev2 = W.run(gm, pcm, 1600)[0], W.run(gm, pcm, 1600, bias=b1)[0], W.run(gm, pcm, 1600, bias=b2)[0]
    assert ev1 != ev0 and ev2 != ev0 and ev1 != ev2
    # one set shared by many sessions, the handle freed while they use it
    evs = [[] for _ in range(8)]
    ss = [A.Session(gm, (lambda q: (lambda t, toks: evs[q].append((t, toks))))(i), raw_events=True, bias=b1) for i in range(8)]
    b1.close()
    g = A.SessionGroup(ss)
    for o in range(0, pcm.size, 1600):
        g.feed([pcm[o:o + 1600]] * 8)
    for s in ss:
        assert s.bias_state()[0] == s.bias_state()[1]
    g.flush()
    assert all(e == ev1 for e in evs)
    # refusal on a busy session
    s = ss[0]
    s.feed_pcm16(pcm[:1600])
    for b in (b2, None):
        with pytest.raises(ValueError):
            s.set_bias(b)
    s.flush()
    s.set_bias(b2)                                                    # ... and accepted after the flush
    for s in ss:
        s.close()

    # set -> off -> another set across flushes on ONE session, against a session with the same audio history that had no set before
    # (the encoder's state does not depend on the search, the search state is reset by the flush)
    def passes(sets):
        e, out = [], []
        q = A.Session(gm, lambda t, toks: e.append((t, toks)), raw_events=True)
        for b in sets:
            q.set_bias(b)
            for o in range(0, pcm.size, 1600):
                q.feed_pcm16(pcm[o:o + 1600])
                assert q.bias_state()[0] == q.bias_state()[1]
            q.flush()
            out.append([(t, toks) for t, toks in e if t == 2]); e.clear()     # FINAL results (the time of the last emission survives a flush and steers provisional tokens)
        q.close()
        return out
    b3 = gm.bias(W.session_phrases(texts, blank, rng))
    a, b = passes([b3, None, b2]), passes([None, None, b2])
    assert a[0] != b[0]
    assert a[1] == b[1], "a session whose set was switched off differs from one that never had a set"
    assert a[2] == b[2] and a[2] != a[1], "a session that changed sets differs from one that got the set first"
    b3.close()
    # slot reuse after aas_free: the next owner of the slot starts at the root with no set
    q_ev = []
    q = A.Session(gm, lambda t, toks: q_ev.append((t, toks)), raw_events=True)
    assert q.bias_state() == (0, 0)
    for o in range(0, pcm.size, 1600):
        q.feed_pcm16(pcm[o:o + 1600])
    assert q.bias_state() == (0, 0)
    q.flush(); q.close()
    assert q_ev == ev0
    assert gm.stats().replay_mismatch == 0
    b2.close(); gm.close()


def test_sixty_four_sets_per_engine(tiny_model):
    """An engine holds 64 different sets: the 65th is refused while all are in use, and accepted -- in the entry that was let go --
    once a session has closed and a flight has released that entry's device copy.  Another model's set is refused by its token list."""
    import april_asr_amd as A
    from april_asr_amd import synth_model as SM
    gm = A.Model(tiny_model["path"])
    texts, blank = W.model_texts(gm), gm.dims.blank_id
    rng = np.random.default_rng(21)
    pcm = W.test_pcm(2.0)[:16000 * 3]
    sets = [gm.bias(W.session_phrases(texts, blank, rng, n=3 + i % 5)) for i in range(65)]
    evs = [[] for _ in range(65)]
    ss = [A.Session(gm, (lambda q: (lambda t, toks: evs[q].append((t, toks))))(i), raw_events=True, bias=sets[i] if i < 64 else None) for i in range(65)]
    with pytest.raises(ValueError):
        ss[64].set_bias(sets[64])
    g = A.SessionGroup(ss[:64])
    g.feed([pcm[:1600]] * 64)                                         # all 64 sets are uploaded and in use
    with pytest.raises(ValueError):
        ss[64].set_bias(sets[64])
    ss[64].set_bias(sets[7])                                          # a set the engine already holds needs no entry
    ss[64].set_bias(None)
    ss[0].close()
    with pytest.raises(ValueError):
        ss[64].set_bias(sets[64])                                     # (the entry is released by the stepping thread, before its next flight)
    g = A.SessionGroup(ss[1:64])
    g.feed([pcm[1600:3200]] * 63)
    ss[64].set_bias(sets[64])
    for o in range(0, pcm.size, 1600):
        ss[64].feed_pcm16(pcm[o:o + 1600])
        assert ss[64].bias_state()[0] == ss[64].bias_state()[1]
    ss[64].flush()
    for s in ss[1:64]:
        s.close()
    assert evs[64] == W.run(gm, pcm, 1600, bias=sets[64])[0]
    ss[64].close()
    # same vocabulary size, another token list
    other = str(os.path.join(os.path.dirname(tiny_model["path"]), "tiny_other_tokens.april"))
    SM.write_model(other, SM.TINY_DIMS, punctuation=False)
    hm = A.Model.load_host_only(other)
    assert hm.dims.vocab == gm.dims.vocab
    ob = hm.bias([W.model_texts(hm)[5] if W.model_texts(hm)[5][:1] == b" " else b" " + W.model_texts(hm)[5]])
    q = A.Session(gm, lambda t, toks: None, raw_events=True)
    with pytest.raises(ValueError):
        q.set_bias(ob)
    q.close()
    assert gm.stats().replay_mismatch == 0
    for b in sets:
        b.close()
    gm.close()
