"""Per-token confidence and top-K alternatives from the device search (aprilx_session_set_confidence).

The float64 statement of the contract and its error bound live in tests/confidence_ref.py (checked on their own by
tests/test_confidence_cpu.py).  Here: the device code against it on given rows, the claim that the option changes no recognition
result, the values live sessions deliver against their own traced logits, one answer bit for bit on every path that reaches the
search, and a C client.  Child processes (fp16 engine, C client) are started once each, with a time limit of their own.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import blank_models as BM
import confidence_ref as R
from conftest import speech_like_pcm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# aprilv0 dimensions, this audio (speech, a silence that crosses the 2.2 s reset, speech again): FINAL results with several tokens
# and provisional tokens both occur (asserted in test_values_in_live_sessions)
LIVE_AUDIO = dict(v0=(12, 13), tiny=(12, 13))


def live_pcm(which, secs=4.0):
    a, b = LIVE_AUDIO[which]
    return np.concatenate([speech_like_pcm(secs, seed=a, silence=(1.5, 1.9)), np.zeros(16000 * 3, np.int16), speech_like_pcm(3.0, seed=b)])


def info_of(raw):
    return None if raw is None else A_ffi().AprilxTokenInfo.from_buffer_copy(raw)


def A_ffi():
    from april_asr_amd import _ffi
    return _ffi


def run(gm, pcm, feed, k, trace=False, mode="sync"):
    """One session over `pcm` in feeds of `feed` samples, then a flush.  Returns (raw events, info log, traced logits or None).
    mode: sync | async | pipelined (aprilx_feed_many_pipelined depth 2)"""
    import april_asr_amd as A
    ev = []
    s = A.Session(gm, lambda t, toks: ev.append((t, toks)), asynchronous=mode == "async", no_rt=mode == "async", raw_events=True,
                  alternatives=k or None)
    assert s.alternatives == k
    s.info_log = []
    if trace:
        s.trace_logits(20000)
    g = A.SessionGroup([s])
    for i in range(0, pcm.size, feed):
        if mode == "pipelined":
            g.feed_pipelined([pcm[i:i + feed]], depth=2)
        else:
            s.feed_pcm16(pcm[i:i + feed])
            if mode == "async":
                s.drain()
    if mode == "pipelined":
        g.drain()
    s.flush()
    if mode == "async":
        s.drain()
    lg = s.traced_logits().copy() if trace else None
    log = s.info_log
    s.close()
    return ev, log, lg


def check_live(ev, log, lg, blank, k):
    """every delivered token's info against the float64 reference on traced row eval_index; returns (tokens checked, FINAL results
    with >= 2 tokens, provisional tokens, worst error / bound)"""
    assert len(ev) == len(log)
    n_tok = n_final2 = n_prov = 0
    worst = 0.0
    for (t, toks), (t2, infos) in zip(ev, log):
        assert t == t2 and len(toks) == len(infos)
        if t == 2 and len(toks) >= 2:
            n_final2 += 1
        for (text, logprob, flags, time_ms), raw in zip(toks, infos):
            assert raw is not None, "a token of an opted-in session without an AprilxTokenInfo"
            info = info_of(raw)
            assert info.size == C.sizeof(A_ffi().AprilxTokenInfo)
            row = lg[int(info.eval_index)]
            worst = max(worst, R.check_info(info, row, blank, k, "evaluation %d" % info.eval_index))
            top = np.float32(info.alt_logit[0])
            assert top.view(np.uint32) == row[int(info.alt_id[0])].view(np.uint32)
            lp = np.float32(logprob)
            if lp.view(np.uint32) != top.view(np.uint32):           # a provisional token: logprob = logit - 8
                assert lp.view(np.uint32) == np.float32(top - np.float32(8.0)).view(np.uint32), (logprob, float(top))
                n_prov += 1
            n_tok += 1
    return n_tok, n_final2, n_prov, worst


# ---------------------------------------------------------------- 1. the device code against float64 on given rows
def same_lane_ids(vocab, blank):
    """Token ids that one lane of the 256 scans (n, n + 256, ...), none of them the blank: [(lower, higher, ...)].
    V >= 500: a pair; V > 768: a triple; V > 1024 (past confidence_row's register window, kConfRegs * 256): a pair 1024 apart -- the
    lower id held in a register, the higher one re-evaluated -- and a pair 256 apart on the two sides of the window."""
    def free(n):
        while any(m == blank for m in range(n % 256, vocab, 256)):
            n += 1
        return n
    out = []
    if vocab >= 500:
        n = free(17)
        out.append((n, n + 256))
    if vocab > 768:
        n = free(45)
        out.append((n, n + 256, n + 512))
    if vocab > 1024 + 64:
        n = free(30)
        out.append((n, n + 1024))
        out.append((n + 768 + 1, n + 1024 + 1))
    for ids in out:
        assert all(0 <= i < vocab and i != blank for i in ids) and len({i % 256 for i in ids}) == 1
    return out


def case_rows(vocab, blank, rng):
    rows = [R.random_rows(rng, 48, vocab, s) for s in (1.0, 10.0, 100.0)]
    extra = []
    t = R.random_rows(rng, 1, vocab, 1.0, offset=0.0)[0]
    top = float(t.max()) + 1.0
    a = t.copy(); a[[3, 7, 11]] = top; extra.append(a)                                    # ties inside K
    a = t.copy(); a[list(range(5, 15))] = top; extra.append(a)                              # a tie across every K boundary
    a = t.copy(); a[[vocab - 1, 2]] = top; a[[9, 20, 21]] = top - 0.5; extra.append(a)      # ties at two levels, first and last lane
    a = t.copy(); a[blank] = top + 5.0; extra.append(a)                                     # the maximum at the blank
    a = t.copy(); a[blank] = top + 5.0; a[[4, 6]] = top; extra.append(a)
    # the blank more than 90 above every other logit: a sum taken around a maximum that leaves the blank out overflows (expf(> 88.7))
    a = t.copy(); a[blank] = top + 95.0; extra.append(a)
    # ties between ids that ONE lane scans: the lower id wins only because ids ascend within a lane and the comparisons are strict
    single = 1 if blank != 1 else 2
    for ids in same_lane_ids(vocab, blank):
        a = t.copy(); a[list(ids)] = top; extra.append(a)                                   # ... as the maximum
        a = t.copy(); a[list(ids)] = top; a[single] = top + 1.0; extra.append(a)            # ... as the second best (offer at k >= 1)
        a = t.copy(); a[list(ids)] = top; a[blank] = top + 5.0; extra.append(a)
    extra.append(np.full(vocab, 2.5, np.float32))                                            # a row of equal values
    extra.append(np.full(vocab, -300.0, np.float32))
    extra.append(np.full(vocab, np.nan, np.float32))                                         # a NaN row
    return np.concatenate(rows + [np.stack(extra)]).astype(np.float32)


def check_kernel_against_float64(gm, what, ks=(1, 4, 8)):
    """aprilx_run_confidence on case_rows against confidence_ref (also what tests/device_optin_mutant_worker.py runs against every
    mutant of confidence_row); returns the worst error / bound ratio"""
    vocab, blank = gm.dims.vocab, gm.dims.blank_id
    rows = case_rows(vocab, blank, np.random.default_rng(vocab))
    worst = 0.0
    for k in ks:
        out = gm.run_confidence(rows, k)
        for i in range(rows.shape[0]):
            assert out[i].size == C.sizeof(A_ffi().AprilxTokenInfo) and out[i].eval_index == i
            worst = max(worst, R.check_info(out[i], rows[i], blank, k, "%s row %d K=%d" % (what, i, k)))
        for ids in same_lane_ids(vocab, blank):                     # (stated here as well: the lower id of a same-lane tie comes first)
            masked = rows.copy(); masked[:, blank] = -np.inf
            hit = [i for i in range(rows.shape[0]) if list(np.flatnonzero(masked[i] == masked[i].max())) == list(ids)]
            assert len(hit) == 2
            for i in hit:
                assert [int(out[i].alt_id[j]) for j in range(min(k, len(ids)))] == list(ids)[:k], (what, i, k, ids)
        eq = rows.shape[0] - 3                                     # the row of equal values: lse = v + log V
        assert abs(float(out[eq].lse) - (2.5 + np.log(vocab))) <= R.lse_bound(2.5 + np.log(vocab))
        assert int(out[eq].n_alt) == min(k, vocab - 1) and [int(out[eq].alt_id[j]) for j in range(out[eq].n_alt)] == [n for n in range(vocab) if n != blank][:k]
        assert int(out[rows.shape[0] - 1].n_alt) == 0 and np.isnan(out[rows.shape[0] - 1].lse)
    return worst


VOCAB = dict(tiny=40, medium=131, v0=500, vocab1100=1100, **{k: v[0] for k, v in BM.MODELS.items()})


@pytest.mark.parametrize("which", ["tiny", "medium", "v0", "vocab1100"] + list(BM.MODELS))
def test_kernel_against_float64(which, request, model_dir):
    import april_asr_amd as A
    from april_asr_amd import synth_model as SM
    if which == "vocab1100":
        path = str(model_dir / "tiny_vocab1100.april")
        SM.write_model(path, dict(SM.TINY_DIMS, vocab=1100))
    else:
        path = BM.model_info(which, request)["path"]
    gm = A.Model(path)
    vocab = gm.dims.vocab
    assert vocab == VOCAB[which] and gm.dims.blank_id == BM.MODELS.get(which, (0, 0))[1]
    worst = check_kernel_against_float64(gm, which)
    print("%s (V = %d): worst error = %.3f of the bound" % (which, vocab, worst))
    with pytest.raises(ValueError):
        gm.run_confidence(case_rows(vocab, gm.dims.blank_id, np.random.default_rng(vocab))[:1], 9)
    gm.close()


# ---------------------------------------------------------------- 2. nothing changes for recognition
@pytest.mark.parametrize("which", ["tiny", "v0"])
def test_nothing_changes_for_recognition(which, request):
    import april_asr_amd as A
    gm = A.Model(request.getfixturevalue(which + "_model")["path"])        # an engine of its own: confidence_records starts at 0
    pcm = live_pcm(which)
    ev0, log0, lg0 = run(gm, pcm, 1600, 0, trace=True)
    ev0g, log0g, _ = run(gm, pcm, 1600, 0)                                   # untraced: the captured graphs
    assert gm.stats().confidence_records == 0, "side records were copied although no session had opted in"
    assert all(raw is None for _, infos in log0 + log0g for raw in infos), "reserved must stay NULL for a session without the option"
    assert any(len(toks) for _, toks in ev0)
    ev4, log4, lg4 = run(gm, pcm, 1600, 4, trace=True)
    assert gm.stats().confidence_records > 0
    ev4g, log4g, _ = run(gm, pcm, 1600, 4)                                   # untraced, through graphs captured after the first opt-in
    ev0h, log0h, _ = run(gm, pcm, 1600, 0)                                   # ... and a session without the option on the same engine
    assert ev0 == ev4 == ev0g == ev4g == ev0h, "the callback sequence depends on the option"
    assert np.array_equal(lg0.view(np.uint32), lg4.view(np.uint32))
    assert all(raw is None for _, infos in log0h for raw in infos)
    assert all(raw is not None for _, infos in log4 + log4g for raw in infos)
    assert log4 == log4g, "eager and graph-replayed steps deliver different confidences"
    assert gm.stats().replay_mismatch == 0
    gm.close()


# ---------------------------------------------------------------- 3. values in live sessions
@pytest.mark.parametrize("which", ["tiny", "v0"])
def test_values_in_live_sessions(which, request):
    import april_asr_amd as A
    gm = A.Model(request.getfixturevalue(which + "_model")["path"])
    pcm = live_pcm(which)
    ev, log, lg = run(gm, pcm, 1600, 4, trace=True)
    n_tok, n_final2, n_prov, worst = check_live(ev, log, lg, gm.dims.blank_id, 4)
    print("%s: %d tokens checked against their traced logits, %d FINAL results with >= 2 tokens, %d provisional tokens; worst error = %.3f of the bound"
          % (which, n_tok, n_final2, n_prov, worst))
    assert n_tok > 0
    if which == "v0":
        assert n_final2 >= 1, "the run must finalise several tokens at once (finalize_before_word / finalize_all paths)"
        assert n_prov >= 1, "the run must deliver a provisional token (the --head_ path)"
    gm.close()


# ---------------------------------------------------------------- 4. one answer on every path, bit for bit
def test_alone_equals_among_63_others(v0_model):
    import april_asr_amd as A
    from oracle import orc_py as O
    gm = A.Model(v0_model["path"])
    pcm = live_pcm("v0")
    ev1, log1, _ = run(gm, pcm, 1600, 4)
    n = 64
    pcms = [pcm] + [O.lcg_pcm16_fast(pcm.size, seed=900 + i) for i in range(1, n)]
    evs = [[] for _ in range(n)]
    ks = [4] + [(1 + i % 8) if i % 2 else 0 for i in range(1, n)]
    ss = [A.Session(gm, (lambda q: (lambda t, toks: evs[q].append((t, toks))))(i), raw_events=True, alternatives=ks[i] or None) for i in range(n)]
    for s in ss:
        s.info_log = []
    g = A.SessionGroup(ss)
    for o in range(0, pcm.size, 1600):
        g.feed([p[o:o + 1600] for p in pcms])
    g.flush()
    assert gm.stats().max_batch_seen == n and gm.stats().replay_mismatch == 0
    assert evs[0] == ev1 and ss[0].info_log == log1, "a session's confidences depend on its neighbours"
    for i in range(1, n):
        for _, infos in ss[i].info_log:
            for raw in infos:
                assert (raw is None) == (ks[i] == 0)
                if raw is not None:
                    assert info_of(raw).n_alt <= ks[i]
    for s in ss:
        s.close()
    gm.close()


def test_feed_sizes_and_delivery_modes_agree(v0_model):
    """100 ms feeds == 40 ms feeds == the whole file in one call (layer-major / offline wavefront with its per-block search graph)
    == the pipelined group feed == an asynchronous session: events and AprilxTokenInfo bytes, eval_index included"""
    import april_asr_amd as A
    gm = A.Model(v0_model["path"])
    pcm = np.concatenate([live_pcm("v0"), speech_like_pcm(10.5, seed=14, silence=(4.0, 7.0))])
    assert pcm.size >= 20 * 16000
    base = run(gm, pcm, 1600, 4)[:2]
    assert sum(len(i) for _, i in base[1]) > 0
    lm0 = gm.stats().lm_chunks
    whole = run(gm, pcm, pcm.size, 4)[:2]
    assert gm.stats().lm_chunks - lm0 >= 400, "the whole-file feed did not take the layer-major path"
    assert whole == base, "whole file in one call"
    assert run(gm, pcm, 640, 4)[:2] == base, "40 ms feeds"
    assert run(gm, pcm, 1600, 4, mode="pipelined")[:2] == base, "pipelined group feed"
    assert run(gm, pcm, 1600, 4, mode="async")[:2] == base, "asynchronous session"
    assert gm.stats().replay_mismatch == 0
    gm.close()


def test_f16_engine(v0_model):
    """fp16 engine (APRIL_PRECISION=f16), in a child process: a session alone == in a batch, values inside the bound against ITS logits"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "confidence_f16_worker.py"), v0_model["path"]],
                       env=dict(os.environ, APRIL_PRECISION="f16"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    print(out[-600:])
    assert r.returncode == 0 and "F16_CONFIDENCE_OK" in out, out[-2000:]


# ---------------------------------------------------------------- 5. K = 8 against K = 2
def test_k8_and_k2_agree_on_what_they_share(v0_model):
    import april_asr_amd as A
    gm = A.Model(v0_model["path"])
    pcm = live_pcm("v0")
    ev2, log2, _ = run(gm, pcm, 1600, 2)
    ev8, log8, _ = run(gm, pcm, 1600, 8)
    assert ev2 == ev8 and len(log2) == len(log8)
    n = 0
    for (_, i2), (_, i8) in zip(log2, log8):
        assert len(i2) == len(i8)
        for a, b in zip(i2, i8):
            a, b = info_of(a), info_of(b)
            assert a.n_alt == 2 and b.n_alt == 8 and a.eval_index == b.eval_index
            for f in ("lse", "token_logprob", "blank_logprob"):
                assert np.float32(getattr(a, f)).view(np.uint32) == np.float32(getattr(b, f)).view(np.uint32), f
            assert list(a.alt_id)[:2] == list(b.alt_id)[:2] and list(a.alt_id)[2:] == [-1] * 6
            assert np.array_equal(np.array(a.alt_logit[:2], np.float32).view(np.uint32), np.array(b.alt_logit[:2], np.float32).view(np.uint32))
            n += 1
    assert n > 0
    gm.close()


# ---------------------------------------------------------------- 6. a C client
def test_c_client_equals_python_binding(v0_model, tmp_path):
    import april_asr_amd as A
    exe = str(tmp_path / "confidence_client")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "confidence_client.cpp"), "-I", os.path.join(ROOT, "include"),
                           "-L", os.path.join(ROOT, "april_asr_amd"), "-laprilasr", "-Wl,-rpath," + os.path.join(ROOT, "april_asr_amd"), "-o", exe])
    pcm = live_pcm("v0")
    path = str(tmp_path / "audio.raw")
    pcm.tofile(path)
    r = subprocess.run([exe, v0_model["path"], path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-1000:]
    gm = A.Model(v0_model["path"])
    ev, log, _ = run(gm, pcm, 1600, 3)
    gm.close()
    want = []
    for t, infos in log:
        want.append("%d %d" % (t, len(infos)))
        for raw in infos:
            i = info_of(raw)
            want.append("%d %08x %08x %d %d" % (i.alt_id[0], np.float32(i.token_logprob).view(np.uint32), np.float32(i.blank_logprob).view(np.uint32), i.eval_index, i.n_alt))
    assert any(" " in l and len(l.split()) == 5 for l in want)
    assert r.stdout.decode().splitlines() == want


def test_python_token_fields(tiny_model):
    import april_asr_amd as A
    gm = A.Model(tiny_model["path"])
    pcm = live_pcm("tiny")
    seen = {0: [], 3: []}
    for k in (0, 3):
        s = A.Session(gm, lambda t, toks, k=k: seen[k].extend(toks), alternatives=k or None)
        for i in range(0, pcm.size, 1600):
            s.feed_pcm16(pcm[i:i + 1600])
        with pytest.raises(ValueError):
            s.set_confidence(2)                    # audio fed since the last flush
        s.flush()
        s.set_confidence(k)                        # allowed again after a completed flush
        s.close()
    assert seen[0] and len(seen[0]) == len(seen[3])
    for a, b in zip(seen[0], seen[3]):
        assert (a.token, a.logprob, a.time) == (b.token, b.logprob, b.time)
        assert a.log_softmax is None and a.confidence is None and a.blank_log_softmax is None and a.alternatives is None
        assert b.log_softmax <= 1e-4 and 0.0 <= b.confidence <= 1.0 + 1e-4 and b.blank_log_softmax <= 1e-4      # (the bound of section 12 at |lse| <= 100)
        assert 1 <= len(b.alternatives) <= 3 and b.alternatives[0][0] == b.token and abs(b.alternatives[0][1] - b.log_softmax) < 1e-6
        assert all(x[1] >= y[1] for x, y in zip(b.alternatives, b.alternatives[1:]))
    gm.close()
