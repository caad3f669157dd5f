"""Worker for tests/test_gpu_tone.py: tone events per session (aprilx_session_set_tones), beside voice activity and DTMF in the same
passes (mode "all3"), and the kernel alone (aprilx_run_tones, aprilx_run_tone_decide), one scenario per process.  Prints one line
"RESULT <json>".
usage: tone_worker.py model.april mode [args ...]

What the detector must give comes from the numpy statement of the contract (tests/tone_ref.py), never from the product; only the
tables and the two libm-derived plan values are the library's (checked against numpy's on the CPU), so that libm differences cannot
leak in."""
import ctypes as C
import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  -- first, so the process uses ONE HIP runtime
import april_asr_amd as A  # noqa: E402
from april_asr_amd import _ffi  # noqa: E402
import tone_ref as R  # noqa: E402
import dtmf_ref as D  # noqa: E402
import input_format_ref as IF  # noqa: E402
from vad_worker import Book, cuts, shift_ms_of  # noqa: E402
from vad_worker import expected as vad_expected  # noqa: E402
from dtmf_worker import expected as dtmf_expected  # noqa: E402
from dtmf_worker import plan_dict as dtmf_plan_dict  # noqa: E402

WAVE_FRAMES = 4                                   # the kernel's frames per wave (csrc/kernels.h kToneWaveFrames)
N_SET = tuple(range(1, 2 * WAVE_FRAMES + 2)) + (64, 65, 257)


def plan_dict(p):
    return dict(W=p.W, k_lo=p.k_lo, F=p.F, half_w=R.F32(p.half_w), min_power=R.F32(p.min_power), second_ratio=R.F32(p.second_ratio),
                min_share=R.F32(p.min_share), bin_hz=R.F32(p.bin_hz), tol_hz=p.tol_hz, on_frames=p.on_frames, off_frames=p.off_frames)


def geometry(m):
    return int(m.dims.sample_rate), int(m.dims.fft_size), int(m.dims.frame_shift), shift_ms_of(m)


def same_bits(a, b):
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def signal_set(rate, w, n, k_lo, f):
    """the signals of the CPU test: single tones on a bin, midway between bins and at both grid edges, the two pairs, noise, speech-like"""
    from conftest import speech_like_pcm
    bin_hz = rate / float(w)
    out = [("on_bin", R.sine((k_lo + 20) * bin_hz, n, rate)), ("midway", R.sine((k_lo + 20.5) * bin_hz, n, rate)),
           ("low_edge", R.sine(k_lo * bin_hz, n, rate)), ("high_edge", R.sine((k_lo + f - 1) * bin_hz, n, rate, -6.0)),
           ("dial", R.pair(350, 440, n, rate)), ("busy", R.pair(480, 620, n, rate, twist_db=-4.0)), ("noise", R.noise(n, -20.0, 4))]
    out = [(name, R.to_pcm(sig + R.noise(n, -55.0, 9))) for name, sig in out]
    sp = speech_like_pcm(max(1.0, n / 16000.0 + 0.1), seed=2)[:n]
    return out + [("speech", np.asarray(sp, np.int16))]


def frame_pool(sr, fft, shift, plan):
    """frames of every signal of the set, 12 of each, then silence, the lowest sample throughout, and random edge samples"""
    rng = np.random.RandomState(11)
    n = 11 * shift + fft
    parts = [R.frames_of(pcm, fft, shift)[:12] for _, pcm in signal_set(sr, plan.W, n, plan.k_lo, plan.F)]
    edge = np.stack([np.zeros(fft, np.int16), np.full(fft, -32768, np.int16), rng.choice(np.array([-32768, 32767, 0, 1, -1], np.int16), size=fft)])
    return np.concatenate(parts + [edge])


def mode_kernel(m):
    sr, fft, shift, sh = geometry(m)
    plan = A.tone_plan(sr, fft, sh)
    p, tab = plan_dict(plan), A.tone_tables(sr, fft)
    pool = frame_pool(sr, fft, shift, plan)
    pool = np.concatenate([pool] * (1 + 300 // len(pool)))
    want_all_r, want_all_p = R.run(p, tab, pool[:257 + 24])
    bad, calls, tonal = [], 0, 0
    for n in N_SET:
        off = 0 if n > 60 else 3 * n                              # (short runs start at different signals)
        fr = pool[off:off + n]
        want_r, want_p = want_all_r[off:off + n], want_all_p[off:off + n]
        rec, pw = m.run_tones([True], [fr])
        calls += 1
        if rec[0].tolist() != want_r.tolist() or not same_bits(pw[0], want_p):
            bad.append(["n%d" % n, int((rec[0] != want_r).any(axis=1).sum()), int((pw[0].view(np.uint32) != want_p.view(np.uint32)).sum())])
        tonal += int((want_r[:, 0] != 0).sum())
    # four runs with different options in ONE launch
    opts = [True, dict(min_level_dbfs=-10.0), dict(second_db=30.0, min_share=0.3), dict(min_share=1.0, min_level_dbfs=-70.0, second_db=3.0)]
    lens, offs = (65, 5, 101, 1), (0, 9, 20, 12)
    frs = [pool[o:o + n] for n, o in zip(lens, offs)]
    rec, pw = m.run_tones(opts, frs)
    calls += 1
    differ = 0
    for r in range(4):
        pr = plan_dict(A.tone_plan(sr, fft, sh, opts[r]))
        want_p = want_all_p[offs[r]:offs[r] + lens[r]]
        want_r = np.array([R.decide(pr, q) for q in want_p], np.uint16).reshape(-1, 2)
        if rec[r].tolist() != want_r.tolist() or not same_bits(pw[r], want_p):
            bad.append(["multi%d" % r, int((rec[r] != want_r).any(axis=1).sum()), int((pw[r].view(np.uint32) != want_p.view(np.uint32)).sum())])
        differ += int(want_r.tolist() != want_all_r[offs[r]:offs[r] + lens[r]].tolist())
    # the decision alone on the edge rows (and on the pool's own powers)
    edges = R.edge_rows(p)
    got = m.run_tone_decide(True, np.stack([q for q, _ in edges]))
    edge_bad = [i for i, (_, want) in enumerate(edges) if tuple(got[i].tolist()) != tuple(want)]
    host_bad = [i for i, (q, want) in enumerate(edges) if tuple(A.tone_decide_host(plan, q)) != tuple(want)]
    calls += 2
    if m.run_tone_decide(True, want_all_p[:120]).tolist() != want_all_r[:120].tolist():
        bad.append(["decide_pool"])
    # refusals of aprilx_run_tones
    L = m._L
    o1 = (_ffi.AprilxToneOptions * 1)(A._tone_options(True))
    n1 = np.array([2], np.int32); fr = np.zeros((2, fft), np.int16); by = np.zeros((2, 2), np.uint16)

    def call(n_runs=1, n=2, size=None):
        n1[0] = n
        o1[0].size = C.sizeof(_ffi.AprilxToneOptions) if size is None else size
        return int(L.aprilx_run_tones(m._handle, C.addressof(o1), n_runs, n1.ctypes.data, fr.ctypes.data, by.ctypes.data, None))
    refusals = [call(n_runs=0), call(n=0), call(n=-1), call(size=8), call()]
    return dict(bad=bad, calls=calls, tonal=tonal, edge_bad=edge_bad, host_bad=host_bad, n_edges=len(edges), differ=differ, refusals=refusals,
                W=plan.W, F=plan.F)


class Run:
    """one session's callbacks (type, token text, logprob bits, flags, time) and its detector events, in delivery order"""

    def __init__(self, m, tones=None, asynchronous=False, **kw):
        self.ev, self.tones, self.keys, self.vad, self.cku = [], [], [], [], 0

        def h(t, toks):
            if int(t) == 3:
                self.cku += 1
            self.ev.append((int(t), [(x[0], struct.pack("<f", float(x[1])), int(x[2]), int(x[3])) for x in toks]))
        self.s = A.Session(m, h, raw_events=True, asynchronous=asynchronous, no_rt=asynchronous, tones=tones,
                           tone_callback=lambda e: self.tones.append((e.kind, e.f1_hz, e.f2_hz, e.time_ms)),
                           dtmf_callback=lambda e: self.keys.append((e.kind, e.digit, e.time_ms)),
                           vad_callback=lambda e: self.vad.append((e.kind, e.time_ms)), **kw)


def expected(p, tab, sh, pcm, fft, shift, seg_ends):
    """records and events of the session's own samples, zero-extended to its real frames; the machine starts afresh after every flush"""
    total = seg_ends[-1]
    need = (total - 1) * shift + fft
    x = np.concatenate([pcm, np.zeros(max(0, need - len(pcm)), np.int16)])
    rec, _ = R.run(p, tab, R.frames_of(x, fft, shift)[:total])
    assert len(rec) == total
    ev, t0 = [], 0
    for end in seg_ends:
        mach = R.machine()
        ev += R.events(p, sh, t0, rec[t0:end], mach) + R.flush(sh, end, mach)
        t0 = end
    return rec, ev


FLUSH_MS = 100 + 500 + 200 + 240                  # inside the first 480 + 620 Hz burst of the scenario


def mode_live(m, mode, chunking):
    sr, fft, shift, sh = geometry(m)
    assert sr == 16000
    asynchronous = mode == "async"
    pcm, _ = R.sequence(R.SCENARIO, sr, -55.0, seed=5)
    pcm8, _ = R.sequence(R.SCENARIO, 8000, -55.0, seed=6)
    other = R.to_pcm(R.sine(700.0, len(pcm), sr, -20.0) * (np.arange(len(pcm)) % 8000 < 3000))      # channel 0 of the two-channel stream: other tones
    assert len(other) == len(pcm) == 2 * len(pcm8)
    # (the second stream takes only tones of 100 ms or more, and its pause of 1000 ms outlasts the silence, the piece of the pair and the
    # 400 ms of zeros behind the 1100 Hz tone: it still holds that tone when the first flush completes)
    opts = [True, dict(min_tone_ms=100, min_pause_ms=1000)]
    plans = [A.tone_plan(sr, fft, sh, o) for o in opts]
    tab = A.tone_tables(sr, fft)
    witht = [Run(m, tones=o, asynchronous=asynchronous) for o in opts]
    twins = [Run(m, asynchronous=asynchronous) for _ in opts]
    tel = Run(m, tones=True, asynchronous=asynchronous, input_sample_rate=8000, input_format="mulaw")
    two = Run(m, tones=True, asynchronous=asynchronous, input_format="s16", channels=2, channel=1)
    tel_raw = IF.encode(pcm8, "mulaw")
    two_raw = np.stack([other, pcm], axis=1).reshape(-1).astype("<i2")
    tel_twin = Run(m, asynchronous=asynchronous, input_sample_rate=8000, input_format="mulaw")
    two_twin = Run(m, asynchronous=asynchronous, input_format="s16", channels=2, channel=1)
    runs, fmt = witht + twins, [tel, two, tel_twin, two_twin]
    grp, fgrp = A.SessionGroup([r.s for r in runs]), A.SessionGroup([r.s for r in fmt])
    before = m.tone_stats()
    books, tel_book = [Book(m.dims) for _ in range(3)], Book(m.dims)
    seg_ends, tel_ends, stream, tel_stream = [], [], [], []
    cut_at = FLUSH_MS * sr // 1000
    for si, (s0, s1) in enumerate([(0, cut_at), (cut_at, len(pcm))]):
        bounds = cuts(s1 - s0, chunking, sr // 10, seed=si)
        bounds = sorted(set(b - b % 2 for b in bounds[:-1]) | {s1 - s0})      # (even: the 8 kHz stream is fed half as many samples)
        for k, (f0, f1) in enumerate(zip(bounds[:-1], bounds[1:])):
            bufs = [pcm[s0 + f0:s0 + f1]] * len(runs)
            fbufs = [tel_raw[(s0 + f0) // 2:(s0 + f1) // 2], two_raw[2 * (s0 + f0):2 * (s0 + f1)]] * 2
            if mode == "sync":
                grp.feed(bufs); fgrp.feed_bytes(fbufs)
            elif mode == "pipe2":
                grp.feed_pipelined(bufs, 2); fgrp.feed_bytes(fbufs, 2)
            else:
                for r, b in zip(runs, bufs):
                    r.s.feed_pcm16(b)
                for r, b in zip(fmt, fbufs):
                    r.s.feed(b)
                if k % 8 == 7:                                # (keeps the ingest queues of asynchronous sessions short)
                    grp.drain(); fgrp.drain()
        grp.flush(); fgrp.flush()
        grp.drain(); fgrp.drain()
        for bk in books:
            bk.feed(s1 - s0); bk.flush()
        seg_ends.append(int(books[0].frames))
        stream += [pcm[s0:s1], np.zeros(6400, np.int16)]
        seg16 = np.asarray(m.resample(IF.decode(tel_raw[s0 // 2:s1 // 2], "mulaw"), 8000), np.int16)      # the telephone stream at the model's rate
        tel_book.feed(len(seg16)); tel_book.flush(); tel_ends.append(int(tel_book.frames))
        tel_stream += [seg16, np.zeros(6400, np.int16)]
    stream, tel_stream = np.concatenate(stream), np.concatenate(tel_stream)
    out = dict(streams=[], twins=[], formatted=[])
    for a, b in list(zip(witht, twins)) + [(tel, tel_twin), (two, two_twin)]:
        fa, fb = a.s.frames(), b.s.frames()
        out["twins"].append(dict(events=a.ev == b.ev, frames=bool(fa.shape == fb.shape and (fa.view(np.uint32) == fb.view(np.uint32)).all()),
                                 chunks=a.s.chunks() == b.s.chunks(), n_events=len(a.ev), n_chunks=a.s.chunks(), twin_tones=len(b.tones),
                                 twin_info=b.s.tone_info() is None))
    for a, plan in zip(witht, plans):
        p = plan_dict(plan)
        rec, want = expected(p, tab, sh, stream, fft, shift, seg_ends)
        want = [list(w) for w in want]
        info = a.s.tone_info()
        got = [list(g) for g in a.tones]
        out["streams"].append(dict(equal=got == want, got=got[:40], want=want[:40], n_want=len(want), frames_seen=info["frames_seen"], real=seg_ends[-1],
                                   tonal_frames=info["tonal_frames"], want_tonal=int((rec[:, 0] != 0).sum()), info_tones=info["tones"],
                                   held=info["held"], W=info["W"], cku=a.cku, names=[R.name(g[1], g[2]) for g in got if g[0] == R.ON],
                                   # the flush inside a held tone: an OFF exactly at the first segment's end
                                   closing=[[g[1], g[2]] for g in got if g[0] == R.OFF and g[3] == seg_ends[0] * sh]))
    p = plan_dict(plans[0])
    for a, x, ends in ((tel, tel_stream, tel_ends), (two, stream, seg_ends)):
        _, want = expected(p, tab, sh, x, fft, shift, ends)
        want = [list(w) for w in want]
        got = [list(g) for g in a.tones]
        info = a.s.tone_info()
        out["formatted"].append(dict(equal=got == want, got=got[:40], want=want[:40], n_want=len(want), frames_seen=info["frames_seen"], real=ends[-1], cku=a.cku))
    after = m.tone_stats()
    out.update(mismatch=int(m.stats().replay_mismatch), launches=after[0] - before[0], tone_frames=after[1] - before[1],
               want_tone_frames=3 * seg_ends[-1] + tel_ends[-1])
    for r in runs + fmt:
        r.s.close()
    return out


ALL_BURSTS = [(0.15, 0.55), (0.9, 1.35)]          # two of vad_worker's bursts ...
ALL_KEYS = [("7", 0.30), ("#", 0.66)]             # ... a key of 100 ms inside the first, and one between them that the flush falls into
ALL_TONES = [((1100,), 1.45, 0.25), ((480, 620), 1.78, 0.15)]      # ... and two tones behind them
ALL_FLUSH_AT = 0.70


def mode_all3(m):
    """all three detectors in the same passes: session 0 with VAD, DTMF and tones, 1 with tones, 2 with DTMF, 3 with none, one group, the
    same samples.  A pass's tone records then sit behind its VAD and DTMF bytes, at an offset rounded up to four"""
    import vad_ref as V
    sr, fft, shift, sh = geometry(m)
    assert sr == 16000
    _, mel = m.fbank_tables()
    sig = V.burst_signal(2.0, ALL_BURSTS, -50.0, 20.0, seed=50).astype(np.int32)
    for d, at in ALL_KEYS:
        tone, onsets = D.digit_signal(d, 100, 0, sr, -200.0, seed=0, tail_ms=0)
        a = int(at * sr)
        sig[a:a + sr // 10] += tone[onsets[0]:onsets[0] + sr // 10]
    for hz, at, dur in ALL_TONES:
        n = int(dur * sr)
        a = int(at * sr)
        sig[a:a + n] += R.to_pcm(R.sine(hz[0], n, sr, -12.0) if len(hz) == 1 else R.pair(hz[0], hz[1], n, sr, -15.0)).astype(np.int32)
    pcm = np.clip(sig, -32768, 32767).astype(np.int16)
    vplan = V.make_plan(mel, sr, sh, V.options())
    dplan = A.dtmf_plan(sr, fft, sh)
    dp, dtab = dtmf_plan_dict(dplan), A.dtmf_tables(sr, dplan.Wd)
    tplan = A.tone_plan(sr, fft, sh)
    tp, ttab = plan_dict(tplan), A.tone_tables(sr, fft)
    runs = [Run(m, tones=t, dtmf=d, vad=v) for v, d, t in ((True, True, True), (None, None, True), (None, True, None), (None, None, None))]
    grp = A.SessionGroup([r.s for r in runs])
    s0_ = [m.vad_stats(), m.dtmf_stats(), m.tone_stats()]
    book, seg_ends, stream, single, odd = Book(m.dims), [], [], 0, 0
    cut_at = int(ALL_FLUSH_AT * sr)
    for si, (s0, s1) in enumerate([(0, cut_at), (cut_at, len(pcm))]):
        bounds = cuts(s1 - s0, "irregular", sr // 10, seed=25 + si)
        for f0, f1 in zip(bounds[:-1], bounds[1:]):
            single += int(f1 - f0 == shift)
            grp.feed([pcm[s0 + f0:s0 + f1]] * len(runs))
        grp.flush(); grp.drain()
        book.feed(s1 - s0); book.flush()
        seg_ends.append(int(book.frames))
        stream += [pcm[s0:s1], np.zeros(6400, np.int16)]
    rows = [r.s.frames() for r in runs]
    if len(rows[0]) != len(book.real):
        raise RuntimeError("the test's frame bookkeeping gives %d ring rows, the session wrote %d" % (len(book.real), len(rows[0])))
    want_vad, _ = vad_expected(vplan, sh, rows[0][np.array(book.real)], seg_ends)
    stream = np.concatenate(stream)
    _, want_keys = dtmf_expected(dp, dtab, sh, stream, fft, shift, seg_ends)
    _, want_tones = expected(tp, ttab, sh, stream, fft, shift, seg_ends)
    s1_ = [m.vad_stats(), m.dtmf_stats(), m.tone_stats()]
    out = dict(vad=[[list(e) for e in r.vad] for r in runs], keys=[[list(e) for e in r.keys] for r in runs], tones=[[list(e) for e in r.tones] for r in runs],
               want_vad=[list(e) for e in want_vad], want_keys=[list(e) for e in want_keys], want_tones=[list(e) for e in want_tones],
               single_frame_feeds=single, events=[r.ev == runs[0].ev for r in runs], n_events=len(runs[0].ev), chunks=[r.s.chunks() for r in runs],
               frames=[bool(x.shape == rows[0].shape and (x.view(np.uint32) == rows[0].view(np.uint32)).all()) for x in rows],
               det_frames=[b[1] - a[1] for a, b in zip(s0_, s1_)], launches=[b[0] - a[0] for a, b in zip(s0_, s1_)], real=seg_ends[-1],
               mismatch=int(m.stats().replay_mismatch))
    for r in runs:
        r.s.close()
    return out


def mode_off(m):
    """an engine where nobody opts in (a session with voice activity and DTMF only): no tone launch, no tone event; then the rules of
    aprilx_session_set_tones, and a profiled pass"""
    sr, fft, shift, sh = geometry(m)
    pcm, _ = R.sequence(R.SCENARIO, sr, -55.0, seed=3)
    out = {}
    plain = Run(m, dtmf=True, vad=True)
    plain.s.feed_pcm16(pcm); plain.s.flush()
    out["unused"] = list(m.tone_stats())
    out["plain_info"] = plain.s.tone_info()
    out["plain_tones"] = len(plain.tones)
    L = m._L
    a = Run(m, tones=True)
    out["fresh"] = a.s.tone_info() is not None

    def raw(size=None, flags=0, handler=True, **kw):
        d = dict(A._TONE_DEFAULTS); d.update(kw)
        o = _ffi.AprilxToneOptions(C.sizeof(_ffi.AprilxToneOptions) if size is None else size, d["min_level_dbfs"], d["second_db"], d["min_share"],
                                   d["tol_hz"], d["min_tone_ms"], d["min_pause_ms"], flags)
        return int(L.aprilx_session_set_tones(a.s._handle, C.byref(o), A._TONE_HANDLER if handler else C.cast(None, _ffi.TONE_HANDLER), id(a.s)))
    out["bad"] = [raw(size=8), raw(flags=2), raw(handler=False), raw(min_level_dbfs=1.0), raw(second_db=2.0), raw(min_share=0.0), raw(tol_hz=0),
                  raw(min_tone_ms=5), raw(min_pause_ms=6000), raw(min_share=float("nan"))]
    out["after_bad"] = a.s.tone_info()["on_frames"]
    out["set"] = raw(min_tone_ms=100)
    out["after_set"] = a.s.tone_info()["on_frames"]
    half = len(pcm) // 2
    a.s.feed_pcm16(pcm[:half])
    out["after_feed"] = raw(min_tone_ms=60)                       # audio fed since the last completed flush: refused
    out["off_after_feed"] = int(L.aprilx_session_set_tones(a.s._handle, None, C.cast(None, _ffi.TONE_HANDLER), None))
    out["still"] = a.s.tone_info()["on_frames"]
    a.s.feed_pcm16(pcm[half:]); a.s.flush()
    out["used"] = list(m.tone_stats())[:2]
    info = a.s.tone_info()
    out["frames_seen"] = info["frames_seen"]
    out["names"] = [R.name(e[1], e[2]) for e in a.tones if e[0] == R.ON]
    out["counters"] = [info["tones"], info["tonal_frames"]]
    out["after_flush"] = raw()
    a.s.set_tones(None)
    out["off"] = a.s.tone_info()
    before = list(m.tone_stats())[:2]
    n_ev = len(a.tones)
    a.s.feed_pcm16(pcm); a.s.flush()
    out["off_launches_nothing"] = list(m.tone_stats())[:2] == before and len(a.tones) == n_ev
    m.profile(1)
    b = Run(m, tones=True)
    b.s.feed_pcm16(pcm); b.s.flush()
    m.profile(0)
    out["profiled_ms"] = m.tone_stats()[2]
    out["profiled_names"] = [R.name(e[1], e[2]) for e in b.tones if e[0] == R.ON]
    out["mismatch"] = int(m.stats().replay_mismatch)
    return out


def main():
    path, mode = sys.argv[1], sys.argv[2]
    m = A.Model(path)
    if mode == "kernel":
        res = mode_kernel(m)
    elif mode == "live":
        res = {c: mode_live(m, sys.argv[3], c) for c in sys.argv[4:]}
    elif mode == "all3":
        res = mode_all3(m)
    else:
        res = mode_off(m)
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
