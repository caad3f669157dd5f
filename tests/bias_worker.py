"""Helpers of tests/test_gpu_bias.py, and -- run as a program -- the whole-session check on an engine of another precision
(APRIL_PRECISION is read when the library loads, so the fp16 engine needs a process of its own):
    python bias_worker.py MODEL.april        prints "ok ..." and exits 0, or raises."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import bias_ref as R  # noqa: E402


def model_texts(gm):
    return [gm._L.aprilx_model_token(gm._handle, i) or b"" for i in range(gm.dims.vocab)]


def test_pcm(seconds=4.0):
    from conftest import speech_like_pcm
    return np.concatenate([speech_like_pcm(seconds, seed=12, silence=(1.5, 1.9)), np.zeros(16000 * 3, np.int16), speech_like_pcm(3.0, seed=13)])


def run(gm, pcm, feed, bias=None, trace=False, mode="sync", k=None, check_state=False):
    """One session over `pcm` in feeds of `feed` samples, then a flush: (raw events, traced logits or None, chunks, info log)."""
    import april_asr_amd as A
    ev = []
    s = A.Session(gm, lambda t, toks: ev.append((t, toks)), raw_events=True, bias=bias, alternatives=k)
    s.info_log = [] if k else None
    if trace:
        s.trace_logits(20000)
    g = A.SessionGroup([s])
    for i in range(0, pcm.size, feed):
        if mode == "pipelined":
            g.feed_pipelined([pcm[i:i + feed]], depth=2)
        else:
            s.feed_pcm16(pcm[i:i + feed])
            if check_state:
                h, d = s.bias_state()
                assert h == d, "trie state: host %d, device %d after the feed at sample %d" % (h, d, i)
    if mode == "pipelined":
        g.drain()
    s.flush()
    assert s.bias_state() == (0, 0)
    out = (ev, s.traced_logits().copy() if trace else None, s.chunks(), s.info_log)
    s.close()
    return out


def replay(gm, texts, ref, lg, chunks, stride_ms=40):
    """The session again from its raw traced logits: bias_ref's search decides, the library's host state machine (aprilx_greedy_*)
    turns the decisions into callbacks.  Returns (events, the rows v' the search compared, the states before each evaluation)."""
    from april_asr_amd import _ffi
    L = gm._L
    blank = gm.dims.blank_id
    ev = []

    def on(ud, t, n, toks):
        ev.append((int(t), [(toks[i].token, float(toks[i].logprob), int(toks[i].flags), int(toks[i].time_ms)) for i in range(n)]))
    cb = _ffi.HANDLER(on)
    g = L.aprilx_greedy_create(gm._handle, cb, None)
    srch = R.Search(R.token_classes(texts), blank, ref)
    row, vps, states = 0, [], []
    for c in range(1, chunks + 1):
        for r in range(3):
            assert row < len(lg), "fewer traced evaluations than the search needs"
            ee = 1.0 if r == 0 else 0.0
            states.append(srch.s)
            vp = ref.biased(lg[row], srch.s) if ref is not None else lg[row]
            vps.append(vp)
            idx, mx, bl = R.argmax_record(vp, blank)
            is_blank = srch.decide(idx, mx, bl, ee, c * stride_ms)
            got = L.aprilx_greedy_step(g, idx, float(mx), float(bl), ee, c * stride_ms, None)
            assert bool(got) == is_blank
            row += 1
            if is_blank:
                break
    assert row == len(lg), "the session evaluated %d rows, the reference search %d" % (len(lg), row)
    L.aprilx_greedy_finish(g)
    L.aprilx_greedy_free(g)
    return ev, vps, states


def same_events(a, b):
    """token for token, logprob bitwise"""
    assert len(a) == len(b), (len(a), len(b))
    for (t0, k0), (t1, k1) in zip(a, b):
        assert t0 == t1 and len(k0) == len(k1)
        for x, y in zip(k0, k1):
            assert x[0] == y[0] and x[2:] == y[2:], (x, y)
            assert np.float32(x[1]).view(np.uint32) == np.float32(y[1]).view(np.uint32), (x, y)


def session_phrases(texts, blank, rng, n=20):
    """phrases of two to four tokens starting at word tokens, boosts large enough to matter against the synthetic logits"""
    words = [i for i, t in enumerate(texts) if t[:1] == b" " and i != blank]
    rest = [i for i, t in enumerate(texts) if t and t[:1] not in (b" ", b"<") and i != blank]
    out = []
    for _ in range(n):
        ids = [int(rng.choice(words))] + [int(rng.choice(rest + words)) for _ in range(int(rng.integers(1, 4)))]
        out.append((b"".join(texts[i] for i in ids), float(np.float32(rng.uniform(1.0, 8.0)))))
    return out


def whole_session(gm, seed=3):
    texts = model_texts(gm)
    blank = gm.dims.blank_id
    phrases = session_phrases(texts, blank, np.random.default_rng(seed))
    ref = R.BiasRef(texts, blank, phrases)
    bias = gm.bias(phrases)
    pcm = test_pcm()
    ev, lg, chunks, _ = run(gm, pcm, 1600, bias=bias, trace=True, check_state=True)
    want, vps, states = replay(gm, texts, ref, lg, chunks)
    same_events(ev, want)
    ev_g, _, _, _ = run(gm, pcm, 1600, bias=bias, check_state=True)          # untraced: the captured graphs
    same_events(ev_g, want)
    ev0, lg0, chunks0, _ = run(gm, pcm, 1600, trace=True)
    same_events(ev0, replay(gm, texts, None, lg0, chunks0)[0])
    assert gm.stats().replay_mismatch == 0
    n_tok = sum(len(t) for _, t in ev)
    moved = sum(1 for s in states if s)
    bias.close()
    return n_tok, moved, ev != ev0


if __name__ == "__main__":
    import torch  # noqa: F401  (one HIP runtime in the process, as tests/conftest.py)
    import april_asr_amd as A
    gm = A.Model(sys.argv[1])
    n_tok, moved, differs = whole_session(gm)
    print("ok precision=%d tokens=%d evaluations_inside_a_phrase=%d differs_from_unbiased=%s" % (gm.dims.precision, n_tok, moved, differs))
    gm.close()
