"""The text-corpus language model without a GPU: the host-side builder (aprilx_lm_create) and walk
(aprilx_lm_score_host) against the numpy statement of the contract in tests/lm_ref.py, a property of the statement itself, the refusals
that need no engine, the host state machine's own copy of the node (aprilx_greedy_set_lm / aprilx_greedy_lm_state), and the builder and
the walk as a stand-alone program under AddressSanitizer + UBSan (tests/cpp/lm_walk_test.cc).  The refusals that need a live session --
a model set mid-stream, the ninth model of an engine, snapshot and restore -- are in tests/test_gpu_lm.py: a session needs an engine."""
import os
import subprocess

import numpy as np
import pytest

import blank_models as BM
import lm_ref as R
import lm_worker as W
import search_options_ref as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "april_asr_amd", "csrc")
SIZES = dict(tiny=40, medium=131, v0=500, blank39=40, blank255=500, blank256=500)


def host_model(request, which):
    import april_asr_amd as A
    info = BM.model_info(which, request)
    m = A.Model.load_host_only(info["path"])
    texts = [t.encode("utf-8") for t in info["tokens"]]
    assert len(texts) == m.dims.vocab == SIZES[which] and m.dims.blank_id == info["blank"] and texts[info["blank"]] == b"<blk>"
    return m, texts


@pytest.mark.parametrize("which", ["tiny", "medium", "v0", "blank39", "blank255", "blank256"])
def test_builder_equals_the_statement(which, request):
    m, texts = host_model(request, which)
    blank = m.dims.blank_id
    rng = np.random.default_rng(len(texts) + blank)
    lines = W.token_lines(texts, blank, rng, 12 if len(texts) > 200 else 20)
    body = W.corpus_of(lines)
    for order in (2, 3, 5, 8):
        lm = m.lm(body, order)
        ref = R.LmRef(texts, blank, body, order)
        W.same_model(lm, ref)
        assert lm.message == "" and lm.dropped_lines == 0
        again = m.lm(body, order).arrays()                 # deterministic: byte-identical for the same input
        assert all(np.asarray(again[k]).tobytes() == np.asarray(v).tobytes() for k, v in lm.arrays().items())
    word = next(t for t in texts if t[:1] == b" " and len(t) > 3)
    cases = {
        "one line": word[1:] + b"\n",
        "no final newline": word[1:],
        "repeated lines": (word[1:] + b"\n") * 5 + lines[0][1:] + b"\n" + (word[1:] + b"\n") * 2,
        "a line shorter than N": word[1:2] + b"\n" + lines[1][1:] + b"\n",
        "a line dropped for a foreign byte": lines[0][1:] + b"\n" + word[1:] + b"\x7f" + b"\n" + b"\xc3\xa9\n" + lines[2][1:] + b"\n",
        "crlf, tabs and runs of spaces": b"\r\n".join(x.replace(b" ", b" \t ") for x in lines[:4]) + b"\r\n\r\n   \t\r\n",
        "leading and trailing spaces": b"  " + lines[3] + b"   \n\n\n" + lines[4] + b"\t\n",
    }
    for name, body in cases.items():
        for order in (2, 5, 8):
            lm = m.lm(body, order)
            ref = R.LmRef(texts, blank, body, order)
            W.same_model(lm, ref)
            if name == "a line dropped for a foreign byte":
                assert lm.dropped_lines == 2 and "2 line(s)" in lm.message
            if name == "a line shorter than N" and order == 8:
                assert ref.nodes > 2


@pytest.mark.parametrize("which", ["tiny", "blank39"])
def test_every_node_is_a_distribution(which, request):
    """a property of the statement itself: sum over the alphabet of P(c | h) is 1 within 1e-12 in float64, for every node"""
    m, texts = host_model(request, which)
    rng = np.random.default_rng(5)
    body = W.corpus_of(W.token_lines(texts, m.dims.blank_id, rng, 20))
    for order in (2, 5, 8):
        ref = R.LmRef(texts, m.dims.blank_id, body, order)
        for h in ref.ctx:
            total = sum(ref.P(c, h) for c in ref.alphabet)
            assert abs(total - 1.0) <= 1e-12, (order, h, total)
        # ... and the automaton's numbers are that distribution: an arc holds ln P, a missing arc costs bow(h) + the shorter context's cost
        for s, h in enumerate(ref.ctx):
            for c in ref.alphabet:
                p, node, cost = ref.P(c, h), s, 0.0
                while c not in ref.cnt[ref.ctx[node]] and node != 0:
                    cost += float(ref.bow[node]); node = int(ref.back[node])
                e = ref._arc[node].get(c)
                cost += float(ref.arc_logp[e]) if e is not None else float(ref.unk_logp)
                assert abs(cost - np.log(p)) <= 1e-5 * max(1.0, abs(np.log(p))), (h, c, cost, np.log(p))


def check_pairs(lm, ref, pairs):
    for s, n in pairs:
        got, want = lm.score(s, n), ref.score(s, n)
        assert W.bits(got[0]) == W.bits(want[0]) and got[1] == want[1], (s, n, got, want)


def test_score_host_all_pairs_v40(request):
    m, texts = host_model(request, "tiny")
    rng = np.random.default_rng(40)
    body = W.corpus_of(W.token_lines(texts, 0, rng, 20))
    for order in (2, 5):
        lm, ref = m.lm(body, order), R.LmRef(texts, 0, body, order)
        check_pairs(lm, ref, [(s, n) for s in range(ref.nodes) for n in range(40)])


def test_score_host_sample_v500(request, model_dir):
    """a seeded sample of 20 000 (node, token) pairs at V = 500 which includes tokens longer than N, tokens with a byte the corpus never
    saw, an empty-text token, the deepest nodes and the start node"""
    import april_asr_amd as A
    from april_asr_amd import synth_model as SM
    request.getfixturevalue("built")
    toks = SM.make_tokens(500)
    empty = 123
    toks[empty] = ""
    path = str(model_dir / "lm_v500_empty.april")
    SM.write_model(path, dict(SM.TINY_DIMS, vocab=500), tokens=toks)
    m = A.Model.load_host_only(path)
    texts = [t.encode() for t in toks]
    rng = np.random.default_rng(500)
    pool = [i for i, t in enumerate(texts) if i and t and i % 3 == 0]            # a third of the tokens: bytes of the others stay unseen
    body = W.corpus_of(W.token_lines(texts, 0, rng, 30, pool=pool))
    order = 3
    lm, ref = m.lm(body, order), R.LmRef(texts, 0, body, order)
    W.same_model(lm, ref)
    seen = set(body)
    unk_tokens = [n for n, t in enumerate(texts) if n and any(c not in seen for c in t)]
    long_tokens = [n for n, t in enumerate(texts) if len(t) > order]
    deepest = [s for s, h in enumerate(ref.ctx) if len(h) == order - 1]
    assert unk_tokens and long_tokens and deepest and texts[empty] == b""
    assert ref.nodes * 500 >= 40000
    pairs = {(int(x) // 500, int(x) % 500) for x in rng.choice(ref.nodes * 500, size=20000, replace=False)}      # 20 000 distinct pairs
    must = [(ref.start, n) for n in unk_tokens[:20] + long_tokens[:20] + [empty]] + [(s, empty) for s in deepest[:5]]
    must += [(s, n) for s in deepest[-40:] for n in (unk_tokens[0], long_tokens[0], long_tokens[-1])]
    pairs = sorted(pairs | set(must))
    assert len(pairs) >= 20000
    check_pairs(lm, ref, pairs)
    assert lm.score(ref.start, empty) == (np.float32(0.0), ref.start)
    # the unk branch really is taken: a byte nobody saw, from the root, costs unk_logp and stays at the root
    n = next(n for n in unk_tokens if texts[n][0] not in seen)
    assert ref.step(0, texts[n][0], np.float32(0.0)) == (0, ref.unk_logp)


def test_refusals_have_messages(request):
    m, texts = host_model(request, "tiny")
    word = next(t for t in texts if t[:1] == b" " and len(t) > 3)[1:]
    for order, what in ((1, "order"), (9, "order"), (0, "order")):
        with pytest.raises(ValueError, match="the order must be 2 .. 8"):
            m.lm(word, order)
        with pytest.raises(R.Refused, match=what):
            R.LmRef(texts, 0, word, order)
    for body in (b"", b"\n\n  \t\r\n", b"\x7f\n\xff\xfe\n"):
        with pytest.raises(ValueError, match="no line of the corpus is left"):
            m.lm(body, 5)
        with pytest.raises(R.Refused):
            R.LmRef(texts, 0, body, 5)
    with pytest.raises(ValueError, match="2 dropped"):
        m.lm(b"\x7f\n\xff\xfe\n", 5)


def test_newline_token_is_refused(request, model_dir):
    import april_asr_amd as A
    from april_asr_amd import synth_model as SM
    request.getfixturevalue("built")
    toks = SM.make_tokens(40)
    toks[9] = "a\nb"
    path = str(model_dir / "lm_newline_token.april")
    SM.write_model(path, SM.TINY_DIMS, tokens=toks)
    m = A.Model.load_host_only(path)
    with pytest.raises(ValueError, match="0x0A"):
        m.lm(b"a b\n", 5)
    with pytest.raises(R.Refused):
        R.LmRef([t.encode() for t in toks], 0, b"a b\n", 5)


def test_options_and_other_token_lists_are_refused(request, capfd):
    """weight and bonus out of range through the entry point that needs no engine (the session's goes through the same check), and a
    model built for another token list"""
    m, texts = host_model(request, "tiny")
    m2, texts2 = host_model(request, "blank39")
    rng = np.random.default_rng(1)
    lm = m.lm(W.corpus_of(W.token_lines(texts, 0, rng, 5)), 3)
    g = W.ProductGreedy(m)
    for w, b, word in ((float("nan"), 0.0, "weight"), (-0.1, 0.0, "weight"), (10.5, 0.0, "weight"), (float("inf"), 0.0, "weight"),
                       (0.3, float("nan"), "bonus"), (0.3, 100.5, "bonus"), (0.3, -101.0, "bonus")):
        assert not R.accepted(w, b)
        capfd.readouterr()
        assert g.L.aprilx_greedy_set_lm(g.g, lm._handle, w, b) == -1
        assert "refused" in capfd.readouterr().err and g.node() == 0
    for w, b in ((0.0, 0.0), (10.0, 100.0), (0.3, -100.0)):
        assert R.accepted(w, b) and g.L.aprilx_greedy_set_lm(g.g, lm._handle, w, b) == 0 and g.node() == lm.start
    g.close()
    # another token list: same size, other texts and blank -- the test-only decision entry refuses before it reaches any engine
    assert m2.dims.vocab == m.dims.vocab
    st = np.zeros((1, 4), np.int32); rec = np.zeros(4, np.int32); lg = np.zeros(40, np.float32); now = np.zeros(1, np.int32); ls = np.zeros(1, np.int32)
    assert m2._L.aprilx_run_decide_lm(m2._handle, 1, 0, lg.ctypes.data, 1.0, now.ctypes.data, 0, st.ctypes.data, rec.ctypes.data, None, None, None,
                                      lm._handle, ls.ctypes.data, 0.3, 0.0) == -1


@pytest.mark.parametrize("which", ["tiny", "blank39"])
def test_greedy_node_follows_the_statement(which, request):
    """the host state machine's own copy of the node through non-blank decisions, blanks, a 2.2 s silence with and without the context
    quirk, a silence under search options, and the end of a flush"""
    m, texts = host_model(request, which)
    blank = m.dims.blank_id
    rng = np.random.default_rng(11)
    body = W.corpus_of(W.token_lines(texts, blank, rng, 20))
    lm, ref = m.lm(body, 5), R.LmRef(texts, blank, body, 5)
    cls = SO.token_classes(texts)
    ids = [n for n in range(len(texts)) if n != blank]
    for opts in (None, (400, 0.0, 0)):
        g = W.ProductGreedy(m, lm, 0.5, 0.25)
        if opts:
            from search_options_worker import make_options
            import ctypes as C
            assert g.L.aprilx_greedy_set_search_options(g.g, C.byref(make_options(opts))) == 0
        node, search = ref.start, SO.Search(cls, blank, opts)
        assert g.node() == node and node != 0
        now, seen_silence, seen_quirk, moved = 0, 0, 0, 0
        for i in range(300):
            tok = int(rng.choice(ids))
            kind = i % 10
            mx, bl = (5.0, 1.0) if kind < 6 else (1.0, 5.0)             # a token, or a blank
            now += 40 if kind != 9 else (500 if opts else 2300)          # every tenth round comes after a silence
            before = list(search.ctx)
            is_blank, silence, _ = search.step(tok, mx, bl, 0.0, now)
            assert g.step(tok, mx, bl, 0.0, now) == is_blank
            if not is_blank:
                node = ref.next(node, tok); moved += 1
            elif silence:
                node = ref.start; seen_silence += 1
                seen_quirk += before[0] == blank and before[1] != blank      # the context is NOT cleared (element 0 is tested): the node returns all the same
            assert g.node() == node, (i, tok, is_blank, silence)
        assert seen_silence >= 20 and moved >= 100
        for tok in ids[:3]:
            now += 40
            g.step(tok, 5.0, 1.0, 0.0, now)
        assert g.node() != ref.start
        g.finish()
        assert g.node() == ref.start
        assert g.L.aprilx_greedy_set_lm(g.g, None, 0.0, 0.0) == 0 and g.node() == 0
        g.close()


def test_walk_and_builder_under_sanitizers(tmp_path):
    """csrc/lm.cc and the walk of csrc/lm.h as a plain host program under AddressSanitizer + UBSan (no GPU, no Python)"""
    exe = str(tmp_path / "lm_walk_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "lm_walk_test.cc"), os.path.join(CSRC, "lm.cc"), "-o", exe], timeout=600)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0 and "all checks passed" in out, out[-3000:]
