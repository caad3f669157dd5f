"""Phrase boosting without a GPU: the host-side builder of a bias set (aprilx_bias_create) against the Python
statement of the contract in tests/bias_ref.py, its refusals, and the host state machine's own copy of the trie state
(aprilx_greedy_set_bias / aprilx_greedy_bias_state) through emissions, a 2.2 s silence and a flush."""
import ctypes as C

import numpy as np
import pytest

import bias_ref as R
import blank_models as BM


def host_model(request, which):
    import april_asr_amd as A
    info = BM.model_info(which, request)
    m = A.Model.load_host_only(info["path"])
    texts = [t.encode("utf-8") for t in info["tokens"]]
    assert len(texts) == m.dims.vocab == dict(tiny=40, medium=131, v0=500, blank39=40, blank255=500)[which]
    assert m.dims.blank_id == info["blank"] and texts[info["blank"]] == b"<blk>"
    return m, texts


def same_csr(bias, ref):
    got, want = bias.csr(), ref.csr()
    assert bias.states == ref.S and bias.n_edges == want[1].size and bias.dropped == ref.dropped
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g, w)
    assert np.array_equal(got[3].view(np.uint32), want[3].view(np.uint32))


def random_phrases(rng, texts, blank, n):
    """phrases assembled from token texts (so that several segmentations can exist), random boosts, some negative, one zero"""
    words = [i for i, t in enumerate(texts) if t[:1] == b" " and i != blank]
    rest = [i for i, t in enumerate(texts) if t[:1] not in (b" ", b"<") and t and i != blank]
    out = []
    for k in range(n):
        ids = [int(rng.choice(words))] + [int(rng.choice(rest + words)) for _ in range(int(rng.integers(0, 4)))]
        boost = 0.0 if k == 1 else float(np.float32(rng.uniform(-3.0, 6.0)))
        out.append((b"".join(texts[i] for i in ids), boost))
    return out


@pytest.mark.parametrize("which", ["tiny", "medium", "v0", "blank39", "blank255"])
def test_builder_equals_the_reference(which, request):
    m, texts = host_model(request, which)
    blank = m.dims.blank_id
    rng = np.random.default_rng(len(texts))
    multi = 0
    for trial in range(6):
        phrases = random_phrases(rng, texts, blank, 3 + 5 * trial)
        if trial == 0:                                     # hand-made: without the leading blank, a shared prefix, a duplicate with another boost
            w = [t for t in texts if t[:1] == b" " and len(t) > 2][:2]
            phrases = [(w[0][1:] + w[1], 2.0), (w[0], 5.0), (w[0] + w[1], -1.0), (w[0][1:] + w[1], 3.0)]
        if trial == 1:                                     # tokens whose text is also the text of two other tokens in a row
            split = [t for t in texts if t[:1] == b" " and any(t[:k] in texts and t[k:] in texts for k in range(2, len(t)))]
            phrases += [(t, 1.5) for t in split[:4]]
        multi += sum(1 for p, _ in phrases if R.segmentations(p if p[:1] == b" " else b" " + p, texts, blank) >= 2)
        b = m.bias(phrases)
        same_csr(b, R.BiasRef(texts, blank, phrases))
        b2 = m.bias(phrases)                               # deterministic: byte-identical arrays for the same phrases in the same order
        for x, y in zip(b.csr(), b2.csr()):
            assert x.tobytes() == y.tobytes()
        tok = np.concatenate([b.edges(s)[0] for s in range(b.states)])
        assert blank not in tok, "the blank never has an edge"
        b.close(); b2.close()
    print("%s: %d tested phrases have two or more segmentations" % (which, multi))
    if which not in ("tiny", "blank39"):                   # (40 tokens: the tiny list has no token that two others spell)
        assert multi >= 1, "at least one tested phrase must have two segmentations into the model's tokens"


def test_hand_derived_case(tiny_model):
    """Two phrases sharing a prefix, one the prefix of the other; every edge listed by hand.  The tokens come from the tiny model's
    list: the test first finds a word-start token ' x' (two bytes) and single letters that exist as tokens of their own."""
    import april_asr_amd as A
    m = A.Model.load_host_only(tiny_model["path"])
    texts = [t.encode() for t in tiny_model["tokens"]]
    ids = {t: i for i, t in enumerate(texts)}
    # the tiny vocabulary (seed 7) holds these; if the generator ever changes, the asserts say so
    need = [b" 1", b"2", b"4"]
    for t in need:
        assert t in ids, (t, texts)
    # phrases " 12" (boost 1) and " 124" (boost 3): trie root -' '-> 1 -'1'-> 2 -'2'-> 3 -'4'-> 4
    b = m.bias([(" 12", 1.0), (" 124", 3.0)])
    assert (b.states, b.dropped) == (5, 0)
    # tokens that can walk: " 1" (root -> 2), "2" (2 -> 3), "4" (3 -> 4); " 3" / "." / ... walk nowhere.  best: nodes 1..3 = 3, node 4 = 3
    t1, t2, t4 = ids[b" 1"], ids[b"2"], ids[b"4"]
    root = [(t1, 2, 3.0)]
    want = {0: root, 1: root, 2: sorted(root + [(t2, 3, 3.0)]), 3: sorted(root + [(t4, 4, 3.0)]), 4: root}
    extra = [i for i, t in enumerate(texts) if t in (b" ", b"1", b" 12", b"12", b"24", b"124", b" 124") and i != 0]
    assert not extra, "the hand-made table assumes these strings are no tokens of the tiny model"
    for s in range(5):
        tok, nxt, bonus = b.edges(s)
        assert [(int(a), int(c), float(d)) for a, c, d in zip(tok, nxt, bonus)] == want[s], s
    # with the prefix phrase boosted MORE than the longer one: best(2), best(3) = 4 (both pass), best(4) = 3
    b = m.bias([(" 12", 4.0), (" 124", 3.0)])
    assert [float(x) for x in b.edges(0)[2]] == [4.0]
    tok, nxt, bonus = b.edges(3)
    assert (int(nxt[list(tok).index(t4)]), float(bonus[list(tok).index(t4)])) == (4, 3.0)
    same_csr(b, R.BiasRef(texts, 0, [(" 12", 4.0), (" 124", 3.0)]))


def test_refusals_and_unspellable(tiny_model):
    import april_asr_amd as A
    m = A.Model.load_host_only(tiny_model["path"])
    texts = [t.encode() for t in tiny_model["tokens"]]
    ok = [t for t in texts if t[:1] == b" "][0]
    for bad, word in (([], "at least one"), ([(b"", 1.0)], "empty"), ([(b" " + b"e" * 256, 1.0)], "longer"), ([(ok, float("nan"))], "finite"),
                      ([(ok, float("inf"))], "finite"), ([(ok, 100.5)], "exceeds"), ([(ok, -101.0)], "exceeds")):
        with pytest.raises(ValueError) as e:
            m.bias(bad)
        assert word in str(e.value), (bad, str(e.value))
        with pytest.raises(R.Refused):
            R.BiasRef(texts, 0, bad)
    m.bias([(ok, 100.0), (ok, -100.0), (ok, 0.0)]).close()                  # the limits themselves are legal
    # a phrase no token sequence can spell ('@' is in no token): no root edge, reported
    b = m.bias([(ok + b"@", 2.0)])
    assert (b.dropped, b.states, b.n_edges) == (1, 1, 0) and "cannot be spelled" in b.message
    b = m.bias([(ok + b"@", 2.0), (ok, 1.0)])
    assert b.dropped == 1 and [float(x) for x in b.edges(0)[2]] and set(float(x) for x in b.edges(0)[2]) == {1.0}
    same_csr(b, R.BiasRef(texts, 0, [(ok + b"@", 2.0), (ok, 1.0)]))
    # the state limit: distinct long phrases over the letters that exist as one-letter tokens
    singles = sorted(t for t in texts if len(t) == 1 and t.isalpha())
    assert len(singles) >= 2
    rng = np.random.default_rng(1)
    many = [(ok + b"".join(singles[int(i)] for i in rng.integers(0, len(singles), 250)), 1.0) for _ in range(300)]
    with pytest.raises(ValueError) as e:
        m.bias(many)
    assert "trie states" in str(e.value)
    with pytest.raises(R.Refused):
        R.BiasRef(texts, 0, many)


def test_edge_limit(v0_model):
    """more than 4 M effective edges: ~60 000 states x the root's edges"""
    import april_asr_amd as A
    m = A.Model.load_host_only(v0_model["path"])
    texts = [t.encode() for t in v0_model["tokens"]]
    words = [t for t in texts if t[:1] == b" " and len(t) >= 2]
    singles = sorted(t for t in texts if len(t) == 1 and t.isalpha())
    assert len(words) >= 100 and len(singles) >= 2
    rng = np.random.default_rng(2)
    many = [(w, 1.0) for w in words] + [(words[0] + b"".join(singles[int(i)] for i in rng.integers(0, len(singles), 240)), 1.0) for _ in range(260)]
    with pytest.raises(ValueError) as e:
        m.bias(many)
    assert "token edges" in str(e.value)


def test_host_state_machine_follows_the_reference(medium_model):
    """scripted (idx, max, blank) sequences through aprilx_greedy_* with a set attached: the state machine's copy of the trie state
    equals bias_ref's after every round -- emissions, blanks, a 2.2 s silence, a flush, set off and on again"""
    import april_asr_amd as A
    from april_asr_amd import _ffi
    m = A.Model.load_host_only(medium_model["path"])
    L = m._L
    texts = [t.encode() for t in medium_model["tokens"]]
    blank = m.dims.blank_id
    rng = np.random.default_rng(5)
    phrases = random_phrases(rng, texts, blank, 12)
    ref = R.BiasRef(texts, blank, phrases)
    bias = m.bias(phrases)
    cb = _ffi.HANDLER(lambda ud, t, n, toks: None)
    g = L.aprilx_greedy_create(m._handle, cb, None)
    assert L.aprilx_greedy_bias_state(g) == 0
    assert L.aprilx_greedy_set_bias(g, bias._handle) == 0
    srch = R.Search(R.token_classes(texts), blank, ref)
    # a walk that follows phrases (so that states deep in the trie are reached), breaks them, and pauses
    now, moved, deep = 0, 0, 0
    ctx = (C.c_int32 * 2)()
    for step in range(4000):
        now += int(rng.choice([40, 40, 40, 400, 2300]))
        e = ref.eff[srch.s]
        if e and rng.random() < 0.7:
            idx = int(rng.choice(sorted(e)))
        else:
            idx = int(rng.integers(1, len(texts)))
        mx = np.float32(rng.normal(0, 3)); bl = np.float32(rng.normal(0, 3))
        ee = float(rng.choice([0.0, 1.0]))
        want_blank = srch.decide(idx, mx, bl, ee, now)
        got_blank = L.aprilx_greedy_step(g, idx, float(mx), float(bl), ee, now, ctx)
        assert bool(got_blank) == want_blank
        assert [ctx[0], ctx[1]] == srch.ctx
        assert L.aprilx_greedy_bias_state(g) == srch.s, step
        moved += srch.s != 0
        deep = max(deep, srch.s)
        if step % 500 == 499:
            L.aprilx_greedy_finish(g); srch.flush()
            assert L.aprilx_greedy_bias_state(g) == 0
    assert moved > 200 and deep > 3
    assert L.aprilx_greedy_set_bias(g, None) == 0 and L.aprilx_greedy_bias_state(g) == 0
    L.aprilx_greedy_step(g, int(sorted(ref.eff[0])[0]), 5.0, -5.0, 0.0, now + 40, ctx)
    assert L.aprilx_greedy_bias_state(g) == 0, "no set, no state"
    L.aprilx_greedy_free(g)
    bias.close()
