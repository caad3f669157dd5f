"""Strict bias sets without a GPU ("strict sets"): the host-side builder (aprilx_bias_create_ex with
APRILX_BIAS_STRICT) against the Python statement in tests/bias_strict_ref.py, byte for byte, on hand-made token lists whose edges
are also listed by hand here -- a dead-end state, a phrase that is lost, restart at terminal states only, a crossing token --,
a non-strict set unchanged, a refused flag; and the host state machine's copy of the trie state with a strict set attached."""
import ctypes as C

import numpy as np
import pytest

import bias_ref as R
import bias_strict_ref as SR

# a hand-made token list for the tiny model's 40 entries; '~nn' fill the rest and occur in no phrase
HAND = ["<blk>", " a", "b", " c", "d", " x", "yz", "w", " xy", "b c", ".", ","]
HAND += ["~%02d" % i for i in range(40 - len(HAND))]
ID = {t: i for i, t in enumerate(HAND)}


@pytest.fixture(scope="module")
def hand(model_dir, built):
    import april_asr_amd as A
    from april_asr_amd import synth_model as SM
    path = str(model_dir / "tiny_hand_tokens.april")
    SM.write_model(path, SM.TINY_DIMS, tokens=HAND)
    m = A.Model.load_host_only(path)
    texts = [t.encode() for t in HAND]
    assert [m._L.aprilx_model_token(m._handle, i) for i in range(40)] == texts and m.dims.blank_id == 0
    return m, texts


def same_csr(bias, ref):
    got, want = bias.csr(), ref.csr()
    assert bias.states == ref.S and bias.n_edges == want[1].size and bias.dropped == ref.dropped
    for g, w in zip(got, want):
        assert g.size == w.size and g.tobytes() == w.astype(g.dtype).tobytes()


def edges(bias, s):
    tok, nxt, bonus = bias.edges(s)
    return [(HAND[int(t)], int(n), float(b)) for t, n, b in zip(tok, nxt, bonus)]


def test_dead_end_state_is_pruned(hand):
    m, texts = hand
    # " xyzw": root -' '-> 1 -x-> 2 -y-> 3 -z-> 4 -w-> 5.  Token " xy" walks to 3, from where no token goes on ("yz" does not start at 3,
    # no token "z" / "zw"): a dead end.  " x" (-> 2), "yz" (2 -> 4), "w" (4 -> 5) spell the phrase.
    p = [(" xyzw", 1.5)]
    loose, strict = m.bias(p), m.bias(p, strict=True)
    assert (" xy", 3, 1.5) in edges(loose, 0), "the boosting set keeps the edge into the dead end"
    assert (strict.flags, strict.strict, loose.flags, strict.states, strict.dropped) == (1, True, 0, 6, 0)
    want = {0: [(" x", 2, 1.5)], 1: [], 2: [("yz", 4, 1.5)], 3: [], 4: [("w", 5, 1.5)], 5: [(" x", 2, 1.5)]}
    for s in range(6):
        assert edges(strict, s) == want[s], s
    same_csr(strict, SR.StrictRef(texts, 0, p))
    again = m.bias(p, strict=True)                          # byte-identical for the same input
    assert all(x.tobytes() == y.tobytes() for x, y in zip(strict.csr(), again.csr()))


def test_lost_phrase_is_counted_and_reported(hand):
    m, texts = hand
    # " xyq": tokens " x" and " xy" walk INTO it, none reaches its end ('q' is in no token): every path it had is gone, it is counted with
    # the unspellable phrases and leaves no state and no edge behind; " ab" stays
    p = [(" xyq", 0.0), (" ab", 0.0)]
    b = m.bias(p, strict=True)
    assert b.dropped == 1 and "1 phrase(s) cannot be spelled" in b.message
    assert b.states == 4 and edges(b, 0) == [(" a", 2, 0.0)] and edges(b, 2) == [("b", 3, 0.0)] and edges(b, 3) == [(" a", 2, 0.0)]
    same_csr(b, SR.StrictRef(texts, 0, p))
    # ... and with no phrase left the set is refused: it would permit nothing (the boosting set of the same input is legal and empty)
    with pytest.raises(ValueError) as e:
        m.bias([(" xyq", 0.0)], strict=True)
    assert "no phrase" in str(e.value)
    with pytest.raises(R.Refused):
        SR.StrictRef(texts, 0, [(" xyq", 0.0)])
    assert m.bias([(" xyq", 0.0)]).n_edges == 0


def test_restart_at_terminal_states_only_and_no_crossing_token(hand):
    m, texts = hand
    # " ab", " abd", " c": 0 -' '-> 1 -a-> 2 -b-> 3* -d-> 4*; 1 -c-> 5*   (* = a phrase ends)
    p = [(" ab", 1.0), (" abd", 3.0), (" c", 2.0)]
    b = m.bias(p, strict=True)
    root = [(" a", 2, 3.0), (" c", 5, 2.0)]
    want = {0: root,
            1: [],                                          # (inside a token: never a state of the search)
            2: [("b", 3, 3.0)],                             # inside a phrase: its continuation and nothing else -- no restart
            3: sorted(root + [("d", 4, 3.0)], key=lambda e: ID[e[0]]),      # " ab" has ended: " abd" may go on, or the next phrase begins
            4: root, 5: root}
    for s in range(6):
        assert edges(b, s) == want[s], s
    loose = m.bias(p)
    assert (" c", 5, 2.0) in edges(loose, 2), "a boosting set restarts anywhere"
    # "b c" would finish " ab" and run on into " c": it walks nowhere whole, so no state permits it
    assert all(ID["b c"] not in b.edges(s)[0] for s in range(b.states))
    same_csr(b, SR.StrictRef(texts, 0, p))
    # a continuation that is pruned does not stand in the way of a restart with the same token: after " a" (a phrase), " xy" towards
    # " a xyzw" is a dead end, but " xy" is also a phrase of its own
    p2 = [(" a", 0.0), (" a xyzw", 0.0), (" xy", 0.0)]
    b2 = m.bias(p2, strict=True)
    assert edges(b2, 0) == [(" a", 2, 0.0), (" xy", 9, 0.0)], "the root's ' x' leads to a dead end (no 'y' token)"
    assert edges(b2, 2) == [(" a", 2, 0.0), (" x", 4, 0.0), (" xy", 9, 0.0)]
    same_csr(b2, SR.StrictRef(texts, 0, p2))
    for ref, set_ in ((SR.StrictRef(texts, 0, p), b), (SR.StrictRef(texts, 0, p2), b2)):
        for s in ref.reachable:
            assert set_.edges(s)[0].size >= 1, "every reachable state permits a token"


def test_non_strict_sets_are_unchanged_and_flags_are_checked(hand):
    m, texts = hand
    L = m._L
    p = [(" ab", 1.0), (" abd", 3.0), (" c", 2.0), (" xyzw", -1.0), (" xyq", 2.0)]
    raw = [x.encode() for x, _ in p]
    arr = (C.c_char_p * len(raw))(*raw)
    boosts = (C.c_float * len(raw))(*[b for _, b in p])
    err = C.create_string_buffer(256)
    old = L.aprilx_bias_create(m._handle, len(raw), arr, boosts, err, 256)
    assert old and L.aprilx_bias_flags(old) == 0 and L.aprilx_bias_flags(None) == -1
    L.aprilx_bias_free(old)
    same_csr(m.bias(p), R.BiasRef(texts, 0, p))             # flags = 0 through aprilx_bias_create_ex: section 13's arrays, byte for byte
    for flags in (2, 3, 0x80000000):
        assert not L.aprilx_bias_create_ex(m._handle, len(raw), arr, boosts, flags, err, 256)
        assert b"unknown flag" in err.value
    import april_asr_amd as A
    with pytest.raises(ValueError):
        A.Bias(m, p, flags=4)


@pytest.mark.parametrize("which", ["tiny", "medium", "v0", "blank39", "blank255"])
def test_builder_equals_the_reference_on_random_sets(which, request):
    import april_asr_amd as A
    import blank_models as BM
    from test_bias_cpu import random_phrases
    info = BM.model_info(which, request)
    m = A.Model.load_host_only(info["path"])
    texts = [t.encode("utf-8") for t in info["tokens"]]
    blank = m.dims.blank_id
    assert blank == info["blank"] and texts[blank] == b"<blk>"
    rng = np.random.default_rng(100 + len(texts))
    for trial in range(5):
        phrases = random_phrases(rng, texts, blank, 3 + 6 * trial)
        ref = SR.StrictRef(texts, blank, phrases)
        b = m.bias(phrases, strict=True)
        same_csr(b, ref)
        loose = m.bias(phrases)
        assert b.n_edges < loose.n_edges and b.states == loose.states
        b.close(); loose.close()


def test_host_state_machine_with_a_strict_set(medium_model):
    """scripted (idx, max, blank) rounds through aprilx_greedy_* with a strict set attached: the state machine's copy of the state equals
    the reference's after every round -- permitted tokens, rounds without a candidate (idx -1), a 2.2 s silence, a flush"""
    import april_asr_amd as A
    from april_asr_amd import _ffi
    from test_bias_cpu import random_phrases
    m = A.Model.load_host_only(medium_model["path"])
    L = m._L
    texts = [t.encode() for t in medium_model["tokens"]]
    blank = m.dims.blank_id
    rng = np.random.default_rng(6)
    phrases = random_phrases(rng, texts, blank, 12)
    ref = SR.StrictRef(texts, blank, phrases)
    bias = m.bias(phrases, strict=True)
    same_csr(bias, ref)
    cb = _ffi.HANDLER(lambda ud, t, n, toks: None)
    g = L.aprilx_greedy_create(m._handle, cb, None)
    assert L.aprilx_greedy_set_bias(g, bias._handle) == 0
    srch = R.Search(R.token_classes(texts), blank, ref)
    now, moved, none = 0, 0, 0
    ctx = (C.c_int32 * 2)()
    for step in range(3000):
        now += int(rng.choice([40, 40, 40, 400, 2300]))
        assert srch.s in ref.reachable and ref.permitted(srch.s), "the search is always at a state that permits a token"
        if rng.random() < 0.1:
            idx, mx = -1, R.INIT                           # nothing permitted beat the initial value
            none += 1
        else:
            idx, mx = int(rng.choice(ref.permitted(srch.s))), np.float32(rng.normal(0, 3))
        bl = np.float32(rng.normal(0, 3))
        ee = float(rng.choice([0.0, 1.0]))
        want_blank = srch.decide(idx, mx, bl, ee, now)
        got_blank = L.aprilx_greedy_step(g, idx, float(mx), float(bl), ee, now, ctx)
        assert bool(got_blank) == want_blank and (idx >= 0 or want_blank), "a round without a candidate resolves to blank"
        assert [ctx[0], ctx[1]] == srch.ctx
        assert L.aprilx_greedy_bias_state(g) == srch.s, step
        moved += srch.s != 0
        if step % 500 == 499:
            L.aprilx_greedy_finish(g); srch.flush()
            assert L.aprilx_greedy_bias_state(g) == 0
    assert moved > 200 and none > 100
    L.aprilx_greedy_free(g)
    bias.close()
