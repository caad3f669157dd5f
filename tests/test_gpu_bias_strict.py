"""Strict bias sets inside the device search ("strict sets"; aprilx_bias_create_ex with APRILX_BIAS_STRICT).

The statement of the contract is tests/bias_strict_ref.py (checked against the host-side builder by tests/test_bias_strict_cpu.py).
Here: the decision kernel on given rows bit for bit (V = 40: one partial pass per lane; V = 500: two passes, the last partial), the
confidences of strict rows over the permitted subset, and live sessions -- strict, boosting and plain ones on one engine.

On the "round that lands in idx = -1" of a LIVE session: a reachable state of a strict set always permits a token (the pruning
guarantees it), and `v > -9999999999` holds for every finite fp32 logit, so a live session of a model with finite logits cannot produce
such a round, however narrow the set; test_live_sessions counts these rounds with the reference over the plain session's traced
logits for its one-phrase set and finds 0 of them, as it must.  The path itself (idx = -1 resolves to blank, the trie state stays) is
pinned on given rows in test_given_rows, where the permitted logits are -inf / NaN."""
import numpy as np
import pytest

import bias_ref as R
import bias_strict_ref as SR
import bias_worker as W
import blank_models as BM
import confidence_ref as CR
from test_gpu_bias import bits, check_rows, decide_plain

pytestmark = pytest.mark.gpu
VALID, BLANK = 1, 2
FINAL, SILENCE = 2, 4


def load(which, request):
    import april_asr_amd as A
    gm = A.Model(BM.model_info(which, request)["path"])
    assert gm.dims.vocab == dict(tiny=40, v0=500, **{k: v[0] for k, v in BM.MODELS.items()})[which]
    assert gm.dims.blank_id == BM.MODELS.get(which, (0, 0))[1]
    return gm


def same_lane_sets(texts, blank, cls):
    """For V >= 500, two strict one- and two-phrase lists whose permitted root tokens meet another id of their own lane (n, n + 256, ...):
    (h, f): h permitted, f = h - 256 forbidden;  (p, q): p and q = p + 256 both permitted.  None below 500 tokens."""
    V = len(texts)
    if V < 500:
        return None
    words = [i for i, t in enumerate(texts) if t[:1] == b" " and len(t) >= 3 and i != blank and not (cls[i] & 22)]
    hf = pq = None
    for h in words:
        f = h - 256
        if hf is None and f >= 0 and f != blank and not (cls[f] & 6):
            ref = SR.StrictRef(texts, blank, [(texts[h], 2.0)])
            if h in ref.permitted(0) and f not in ref.permitted(0):
                hf = (h, f, ref)
        q = h + 256
        if pq is None and q in words:
            ref = SR.StrictRef(texts, blank, [(texts[h], 2.0), (texts[q], 2.0)])
            if h in ref.permitted(0) and q in ref.permitted(0):
                pq = (h, q, ref)
    assert hf is not None and pq is not None, "the vocabulary has no word tokens 256 apart"
    return hf, pq


def pick_tokens(texts, blank, cls):
    """word tokens a, b, c (no punctuation, none the prefix of another's text) and a phrase list over them"""
    words = [i for i, t in enumerate(texts) if t[:1] == b" " and len(t) >= 3 and i != blank and not (cls[i] & 22)]
    out = []
    for i in words:
        if all(not texts[i].startswith(texts[j]) and not texts[j].startswith(texts[i]) for j in out):
            out.append(i)
        if len(out) == 3:
            return out
    raise AssertionError("the vocabulary has no three independent word tokens")


# ---------------------------------------------------------------- 1. the decision kernel on given rows
@pytest.mark.parametrize("which", ["tiny", "v0", "blank64", "blank255", "blank1050"])
def test_given_rows(which, request):
    gm = load(which, request)
    check_given_rows(gm)
    gm.close()


def check_given_rows(gm):
    """the decision kernel with strict sets on hand-made rows and random rounds against bias_strict_ref, bit for bit (also what
    tests/device_optin_mutant_worker.py runs against every mutant of the bias lines)"""
    texts, blank, V = W.model_texts(gm), gm.dims.blank_id, gm.dims.vocab
    cls = R.token_classes(texts)
    a, b, c = pick_tokens(texts, blank, cls)
    phrases = [(texts[a] + texts[b], 2.0), (texts[c], 2.0)]
    ref, bias = SR.StrictRef(texts, blank, phrases), gm.bias(phrases, strict=True)
    assert bias.strict and np.array_equal(bias.csr()[1], ref.csr()[1])
    perm0 = ref.permitted(0)
    s_ab = min(s for s in ref.reachable if len(ref.permitted(s)) == 1)      # inside the first phrase, where only its continuation is left
    one = ref.permitted(s_ab)
    assert a in perm0 and c in perm0 and s_ab != 0
    forb = [n for n in range(V) if n != blank and n not in perm0 and n not in one and not (cls[n] & 6)]
    f_lo, f_hi = forb[0], forb[-1]
    assert f_lo < a and (V < 256 or f_hi >= 256), "a forbidden token below the permitted one (it would win a tie), one in the last pass"
    ctx_tok = forb[1]

    def row(vals, fill=-20.0):
        r = np.full(V, fill, np.float32)
        r[blank] = -10.0
        for n, v in vals.items():
            r[n] = v
        return r
    inf = np.float32(np.inf)
    cases = [   # (what, row, state, idx expected, blank expected)
        ("the raw arg-max is forbidden", row({f_lo: 9.0, f_hi: 8.0, a: 3.0}), 0, a, False),
        ("tie between a permitted and a forbidden token with the lower id", row({f_lo: 5.0, a: 3.0}), 0, a, False),      # 3 + 2 == 5
        ("tie of raw logits", row({f_lo: 5.0, f_hi: 5.0, a: 5.0, c: 4.0}), 0, a, False),
        ("a state with exactly one permitted token", row({}, fill=7.0), s_ab, one[0], False),
        ("one permitted token, and it loses to the blank", row({blank: 30.0}, fill=7.0), s_ab, one[0], True),
        ("nothing permitted is finite: -inf", row({**{n: -inf for n in perm0}, f_lo: 9.0}), 0, -1, True),
        ("nothing permitted is finite: NaN", row({one[0]: np.nan, f_hi: 9.0}), s_ab, -1, True),
        ("a permitted token at the initial value does not beat it", row({one[0]: R.INIT - np.float32(2.0)}), s_ab, -1, True),
    ]
    assert bits(np.float32(3.0) + np.float32(2.0)) == bits(np.float32(5.0))
    for what, r, s, want_idx, want_blank in cases:
        srch = R.Search(cls, blank, ref)
        srch.ctx = [blank, ctx_tok]; srch.s = s
        plain = R.Search(cls, blank, None)
        plain.ctx = [blank, ctx_tok]
        rec, _ = check_rows(gm, ref, bias, [srch, plain], np.stack([r, r]), 0.0, np.array([40, 40], np.int32), 0, what)
        assert int(rec["idx"][0]) == want_idx and bool(rec["flags"][0] & BLANK) == want_blank, (what, rec[0])
        if want_idx < 0:
            assert srch.s == s, "a round without a candidate leaves the trie state alone"
        alone, _ = decide_plain(gm, r[None], 0.0, [40], 0, [[blank, ctx_tok, -1, 0]])
        assert rec[1].tobytes() == alone[0].tobytes(), "a row without a set differs from aprilx_run_decide: " + what

    # ---- ties inside one lane of bias_scan (ids 256 apart), V >= 500
    lanes = same_lane_sets(texts, blank, cls)
    if lanes:
        (h, f, ref_h), (p, q, ref_pq) = lanes
        bias_h, bias_pq = gm.bias([(texts[h], 2.0)], strict=True), gm.bias([(texts[p], 2.0), (texts[q], 2.0)], strict=True)
        tie_cases = [
            ("a tie after the bonus between a permitted id and the forbidden id 256 below it", ref_h, bias_h, row({f: 5.0, h: 3.0}), h),
            ("the forbidden id 256 below the permitted one is the raw arg-max", ref_h, bias_h, row({f: 9.0, h: 3.0}), h),
            ("a tie of two permitted ids 256 apart", ref_pq, bias_pq, row({p: 3.0, q: 3.0}), p),
            ("two permitted ids 256 apart, the higher one ahead", ref_pq, bias_pq, row({p: 3.0, q: 3.5}), q),
        ]
        for what, rf, bs, r, want_idx in tie_cases:
            srch = R.Search(cls, blank, rf)
            srch.ctx = [blank, ctx_tok]
            rec, _ = check_rows(gm, rf, bs, [srch], r[None], 0.0, np.array([40], np.int32), 0, what)
            assert int(rec["idx"][0]) == want_idx and not (rec["flags"][0] & BLANK), (what, rec[0])
            assert bits(rec["max"][0]) == bits(np.float32(r[want_idx]) + np.float32(2.0))
        bias_h.close(); bias_pq.close()

    # ---- random rounds: 24 rows per launch (every fourth without a set), 12 launches in sequence, three rounds, silences
    rng = np.random.default_rng(V)
    phrases = W.session_phrases(texts, blank, rng, n=12)
    ref2, bias2 = SR.StrictRef(texts, blank, phrases), gm.bias(phrases, strict=True)
    searches = [R.Search(cls, blank, ref2 if i % 4 else None) for i in range(24)]
    now = np.zeros(24, np.int32)
    moved = forbidden_max = 0
    for step in range(12):
        rows = rng.normal(0.0, 2.0, (24, V)).astype(np.float32)
        rows[:, blank] += 1.0
        for i, s in enumerate(searches):
            if s.ref is not None:
                forbidden_max += int(np.nanargmax(np.where(np.arange(V) == blank, -np.inf, rows[i]))) not in ref2.eff[s.s]
        now += rng.choice([40, 40, 80, 2300], 24).astype(np.int32)
        rnd = int(rng.integers(0, 3))
        check_rows(gm, ref2, bias2, searches, rows, 1.0 if rnd == 0 else 0.0, now, rnd, "random step %d" % step)
        moved += sum(1 for s in searches if s.s)
    assert moved > 20 and forbidden_max > 100, "the rounds must reach states inside phrases, with the raw arg-max forbidden"

    # ---- a boosting (non-strict) set and rows without a set in one launch: each row equals the same row launched alone
    loose_ref, loose = R.BiasRef(texts, blank, phrases), gm.bias(phrases)
    rows = rng.normal(0.0, 2.0, (8, V)).astype(np.float32)
    states = [loose_ref.next(0, sorted(loose_ref.eff[0])[i % len(loose_ref.eff[0])]) if i % 2 else -1 for i in range(8)]
    st = np.tile(np.array([blank, ctx_tok, -1, 0], np.int32), (8, 1))
    now8 = np.full(8, 40, np.int32)
    rec, st2, bs2 = gm.run_decide_biased(rows, 1.0, now8, 0, st, loose, states)
    for i in range(8):
        r1, s1, b1 = gm.run_decide_biased(rows[i:i + 1], 1.0, now8[:1], 0, st[:1], loose, states[i:i + 1])
        assert rec[i].tobytes() == r1[0].tobytes() and st2[i].tobytes() == s1[0].tobytes() and bs2[i] == b1[0], i
        if states[i] < 0:
            p, _ = decide_plain(gm, rows[i:i + 1], 1.0, [40], 0, st[:1])
            assert rec[i].tobytes() == p[0].tobytes(), i
        else:
            idx, mx, bl = R.argmax_record(loose_ref.biased(rows[i], states[i]), blank)
            assert int(rec["idx"][i]) == idx and bits(rec["max"][i]) == bits(mx) and bits(rec["blank"][i]) == bits(bl)
    for x in (bias, bias2, loose):
        x.close()


# ---------------------------------------------------------------- 2. confidences of strict rows
@pytest.mark.parametrize("which", ["tiny", "v0", "blank39", "blank1050"])
def test_confidences_over_the_permitted_subset(which, request):
    gm = load(which, request)
    check_confidences_over_the_permitted_subset(gm)
    gm.close()


def check_confidences_over_the_permitted_subset(gm):
    texts, blank, V = W.model_texts(gm), gm.dims.blank_id, gm.dims.vocab
    rng = np.random.default_rng(7 * V)
    phrases = W.session_phrases(texts, blank, rng, n=12)
    ref, bias = SR.StrictRef(texts, blank, phrases), gm.bias(phrases, strict=True)
    K = 4
    by_count = {}
    for s in sorted(ref.reachable):
        by_count.setdefault(min(len(ref.permitted(s)), K), s)
    assert {1, K} <= set(by_count), "states with one and with at least K permitted tokens"
    states = [by_count[k] for k in sorted(by_count)] * 3 + [0]
    n = len(states)
    rows = CR.random_rows(rng, n, V, 3.0, offset=50.0)
    rows[-1, ref.permitted(0)] = np.nan                      # a row with nothing permitted: n_alt 0, lse NaN
    out = gm.run_confidence_biased(rows, K, bias, states)
    st = np.tile(np.array([blank, blank, -1, 0], np.int32), (n, 1))
    rec, _, _ = gm.run_decide_biased(rows, 1.0, np.zeros(n, np.int32), 0, st, bias, states)
    worst, seen = 0.0, set()
    for i, s in enumerate(states):
        lse64, ids, logits, n_alt = SR.confidence(ref, rows[i], s, K)
        info = out[i]
        assert int(info.n_alt) == n_alt == (0 if i == n - 1 else min(K, len(ref.permitted(s)))), (i, s, int(info.n_alt), n_alt)
        seen.add(n_alt)
        if n_alt == 0:
            assert np.isnan(info.lse) and int(rec["idx"][i]) == -1
            continue
        got = [int(info.alt_id[j]) for j in range(n_alt)]
        assert got == [int(x) for x in ids] and set(got) <= set(ref.permitted(s)), (i, got, ids)
        assert [int(info.alt_id[j]) for j in range(n_alt, 8)] == [-1] * (8 - n_alt)
        assert np.array_equal(bits(np.array([info.alt_logit[j] for j in range(n_alt)], np.float32)), bits(logits))
        assert int(info.alt_id[0]) == int(rec["idx"][i]) and bits(info.alt_logit[0]) == bits(rec["max"][i])
        ratio = abs(float(info.lse) - lse64) / CR.lse_bound(lse64)
        assert ratio <= 1.0, "row %d state %d: lse %r vs %r: %.3g of the bound" % (i, s, float(info.lse), lse64, ratio)
        full = CR.reference(rows[i], blank, K)[0]
        if len(ref.permitted(s)) < V // 2:
            assert abs(full - lse64) > 10 * CR.lse_bound(lse64), "the check must tell the permitted subset from the whole row"
        worst = max(worst, ratio)
    print("V = %d: %d strict rows, n_alt seen %s, worst lse error %.3f of the bound" % (V, n, sorted(seen), worst))
    assert {0, 1, K} <= seen
    # rows with a boosting set and rows without one through the same kernel: section 12 on v' / v, as before
    loose_ref, loose = R.BiasRef(texts, blank, phrases), gm.bias(phrases)
    st2 = [0, -1, loose_ref.next(0, sorted(loose_ref.eff[0])[0]), -1]
    out2 = gm.run_confidence_biased(rows[:4], K, loose, st2)
    for i, s in enumerate(st2):
        CR.check_info(out2[i], loose_ref.biased(rows[i], s) if s >= 0 else rows[i], blank, K, "boosting / plain row %d" % i)
    bias.close(); loose.close()


# ---------------------------------------------------------------- 3. live sessions
def run_group(gm, pcm, sets, trace=()):
    """one session per entry of `sets` (a Bias or None), all fed `pcm` in 100 ms feeds as one group, then flushed"""
    import april_asr_amd as A
    evs = [[] for _ in sets]
    ss = [A.Session(gm, (lambda q: (lambda t, toks: evs[q].append((t, toks))))(i), raw_events=True, bias=b) for i, b in enumerate(sets)]
    for i in trace:
        ss[i].trace_logits(20000)
    g = A.SessionGroup(ss)
    for o in range(0, pcm.size, 1600):
        g.feed([pcm[o:o + 1600]] * len(ss))
        for s, b in zip(ss, sets):
            h, d = s.bias_state()
            assert h == d and (b is not None or h == 0), "trie state: host %d, device %d" % (h, d)
    g.flush()
    lg = {i: (ss[i].traced_logits().copy(), ss[i].chunks()) for i in trace}
    for s in ss:
        assert s.bias_state() == (0, 0)
        s.close()
    return evs, lg


def test_live_sessions(tiny_model):
    import april_asr_amd as A
    gm = A.Model(tiny_model["path"])
    texts, blank = W.model_texts(gm), gm.dims.blank_id
    cls = R.token_classes(texts)
    ids = {t: i for i, t in enumerate(texts)}
    rng = np.random.default_rng(31)
    phrases = W.session_phrases(texts, blank, rng, n=10)
    narrow = [(texts[pick_tokens(texts, blank, cls)[0]], 0.0)]            # ONE phrase of one token
    loose = gm.bias(phrases)
    pcm = W.test_pcm()
    before, lg0 = run_group(gm, pcm, [loose, None], trace=(1,))           # no strict session has been on this engine yet
    # the synthetic model's blank wins nearly every round; a boost larger than the whole logit spread of the plain run lets the permitted
    # tokens win, so that the strict sessions deliver tokens to check (as test_gpu_bias.py's test_effect_on_the_transcript)
    boost = min(100.0, 2.0 * float(np.ceil(lg0[1][0].max() - lg0[1][0].min())))
    wide = [(p, boost) for p, _ in phrases]
    narrow = [(narrow[0][0], boost)]
    refs = [SR.StrictRef(texts, blank, wide), SR.StrictRef(texts, blank, narrow)]
    strict = [gm.bias(wide, strict=True), gm.bias(narrow, strict=True)]
    evs, lg = run_group(gm, pcm, [strict[0], loose, strict[1], None], trace=(0, 2))
    assert evs[1] == before[0] and evs[3] == before[1], "the boosting and the plain session changed when strict sessions joined"
    after, _ = run_group(gm, pcm, [loose, None])
    assert after == before
    for k, ref in ((0, refs[0]), (2, refs[1])):
        # the session again from its raw traced logits, decided by the reference: the same callbacks, bit for bit
        want, vps, states = W.replay(gm, texts, ref, lg[k][0], lg[k][1])
        W.same_events(evs[k], want)
        # every delivered token is a permitted continuation: the reference's state walked over the transcript alone
        s = n_tok = 0
        for t, toks in evs[k]:
            if t == SILENCE:
                s = 0
            if t != FINAL:
                continue
            for tok in toks:
                n = ids[tok[0]]
                assert n in ref.eff[s], "session %d delivered %r, which state %d does not permit" % (k, tok[0], s)
                s = ref.next(s, n)
                n_tok += 1
        raw_forbidden = sum(1 for v, st in zip(lg[k][0], states) if R.argmax_record(v, blank)[0] not in ref.eff[st])
        print("strict session %d: %d tokens delivered, %d of %d evaluations had a forbidden raw arg-max" % (k, n_tok, raw_forbidden, len(states)))
        assert n_tok > 0 and raw_forbidden > 0, "the set must matter in this run"
    assert evs[0] != evs[3] and evs[2] != evs[3] and evs[0] != evs[2]
    # rounds without a candidate, counted by the reference over the PLAIN session's traced logits with the one-phrase set: none, and
    # there can be none (see the head of this file) -- every logit is finite, the one permitted token always beats the initial value
    plain_lg = lg0[1][0]
    assert np.isfinite(plain_lg).all()
    none = sum(1 for v in plain_lg for s in refs[1].reachable if R.argmax_record(refs[1].biased(v, s), blank)[0] < 0)
    assert none == 0
    assert gm.stats().replay_mismatch == 0
    for b in strict + [loose]:
        b.close()
    gm.close()
