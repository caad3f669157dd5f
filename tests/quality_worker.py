"""Worker for tests/test_gpu_quality.py: line quality per session (aprilx_session_set_quality), beside the three detectors in the same
passes (mode "all4"), and the kernel alone (aprilx_run_quality), one scenario per process.  Prints one line "RESULT <json>".
usage: quality_worker.py model.april mode [args ...]

What the observer must give comes from the numpy statement of the contract (tests/quality_ref.py), never from the product."""
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
import quality_ref as R  # noqa: E402
import input_format_ref as IF  # noqa: E402
from vad_worker import Book, cuts, shift_ms_of  # noqa: E402

N_SET = (1, 3, 4, 5, 257)                         # the edges of four frames per workgroup, and a run several workgroups walk in strides
LEVELS = (32767, 32124, 1024)


def geometry(m):
    return int(m.dims.sample_rate), int(m.dims.fft_size), int(m.dims.frame_shift), shift_ms_of(m)


def frame_pool(fft, hop, seed=1):
    """frames of fft samples whose hop is: random int16; quiet noise; zeros; a stuck 1234; the lowest sample throughout; alternating full
    scale; runs below and at clip_run_min, across samples 63 | 64 and up to H - 1, at L - 1, L and -L; the extreme sample in lane 63 and
    at H - 1.  What lies behind the hop is random and must not count."""
    rng = np.random.RandomState(seed)
    L = 32124
    hops = [rng.randint(-32768, 32768, size=hop) for _ in range(8)] + [rng.randint(-30, 31, size=hop) for _ in range(3)]
    hops += [np.zeros(hop), np.full(hop, 1234), np.full(hop, -32768), np.where(np.arange(hop) % 2 == 0, 32767, -32767)]
    for at, n, v in ((5, 2, L), (5, 3, L), (61, 6, L), (hop - 2, 2, L), (0, hop, 32767), (5, 3, L - 1), (5, 3, -L), (hop - 3, 3, 32767), (62, 3, -32768)):
        x = rng.randint(-900, 901, size=hop)
        x[at:at + n] = v
        hops.append(x)
    for at, v in ((63, 32767), (63, -32768), (hop - 1, 32767), (hop - 1, -32768), (0, 32767)):      # the extreme in lane 63, at H - 1, in lane 0
        x = rng.randint(-900, 901, size=hop)
        x[at] = v
        hops.append(x)
    x = np.zeros(hop); x[hop - 1] = 1                                  # dead but for the last sample
    hops.append(x)
    fr = rng.randint(-32768, 32768, size=(len(hops), fft)).astype(np.int16)
    for i, h in enumerate(hops):
        fr[i, :hop] = np.asarray(h, np.int16)
    return fr


def mode_kernel(m):
    sr, fft, hop, sh = geometry(m)
    pool = frame_pool(fft, hop)
    pool = np.concatenate([pool] * (1 + 300 // len(pool)))
    want = {lv: R.run(hop, lv, pool[:300]) for lv in LEVELS}
    host_bad = [lv for lv in LEVELS if A.quality_host(hop, lv, pool[:300]).tolist() != want[lv].tolist()]
    bad, calls = [], 0
    for n in N_SET:
        for k, lv in enumerate(LEVELS):
            off = 0 if n > 40 else (7 * n + 3 * k) % 30
            rec = m.run_quality([lv], [pool[off:off + n]])
            calls += 1
            if rec[0].tolist() != want[lv][off:off + n].tolist():
                bad.append(["n%d_L%d" % (n, lv), int((rec[0] != want[lv][off:off + n]).any(axis=1).sum())])
    # the whole pool once, so that every special frame has gone through the kernel
    n_pool = len(frame_pool(fft, hop))
    rec = m.run_quality([32124], [pool[:n_pool]])
    calls += 1
    if rec[0].tolist() != want[32124][:n_pool].tolist():
        bad.append(["pool", np.nonzero((rec[0] != want[32124][:n_pool]).any(axis=1))[0].tolist()])
    # three runs with different clip levels in ONE launch
    lens, offs = (5, 257, 3), (0, 2, 11)
    rec = m.run_quality(LEVELS, [pool[o:o + n] for n, o in zip(lens, offs)])
    calls += 1
    differ = 0
    for r in range(3):
        w = want[LEVELS[r]][offs[r]:offs[r] + lens[r]]
        if rec[r].tolist() != w.tolist():
            bad.append(["multi%d" % r, int((rec[r] != w).any(axis=1).sum())])
        differ += int(w.tolist() != want[32767][offs[r]:offs[r] + lens[r]].tolist())
    # refusals of aprilx_run_quality
    L = m._L
    lv1 = np.array([32767], np.int32); n1 = np.array([2], np.int32); fr = np.zeros((2, fft), np.int16); out = np.zeros((2, 8), np.uint32)

    def call(n_runs=1, n=2, level=32767):
        n1[0], lv1[0] = n, level
        return int(L.aprilx_run_quality(m._handle, lv1.ctypes.data, n_runs, n1.ctypes.data, fr.ctypes.data, out.ctypes.data))
    refusals = [call(n_runs=0), call(n=0), call(n=-1), call(level=1023), call(level=32768), call()]
    return dict(bad=bad, calls=calls, host_bad=host_bad, differ=differ, refusals=refusals, hop=hop, clipped=int((want[32124][:, 4] >> 16 >= 3).sum()),
                dead=int(want[32124][:, 5].sum()))


class Run:
    """one session's callbacks (type, token text, logprob bits, flags, time) and its detector events, in delivery order"""

    def __init__(self, m, quality=None, asynchronous=False, **kw):
        self.ev, self.q, self.tones, self.keys, self.vad, self.cku = [], [], [], [], [], 0

        def h(t, toks):
            if int(t) == 3:
                self.cku += 1
            self.ev.append((int(t), [(x[0], struct.pack("<f", float(x[1])), int(x[2]), int(x[3])) for x in toks]))
        self.s = A.Session(m, h, raw_events=True, asynchronous=asynchronous, no_rt=asynchronous, quality=quality,
                           quality_callback=lambda e: self.q.append(e.astuple()),
                           tone_callback=lambda e: self.tones.append((e.kind, e.f1_hz, e.f2_hz, e.time_ms)),
                           dtmf_callback=lambda e: self.keys.append((e.kind, e.digit, e.time_ms)),
                           vad_callback=lambda e: self.vad.append((e.kind, e.time_ms)), **kw)


def scenario(sr, seed):
    """2.6 s: a 440 Hz tone with a slow envelope around -20 dBFS over a noise floor and a DC offset; 0.30 .. 0.45 s overdriven into the
    rails; digital silence 0.90 .. 1.25 s; a stuck value 1.60 .. 1.90 s"""
    rng = np.random.RandomState(seed)
    n = int(2.6 * sr)
    t = np.arange(n) / float(sr)
    sig = 0.1 * np.sin(2 * np.pi * 440.0 * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) + rng.normal(0, 10 ** (-50 / 20.0), size=n) + 0.01
    a, b = int(0.30 * sr), int(0.45 * sr)
    sig[a:b] *= 20.0
    pcm = np.clip(np.round(sig * 32768.0), -32768, 32767).astype(np.int16)
    pcm[int(0.90 * sr):int(1.25 * sr)] = 0
    pcm[int(1.60 * sr):int(1.90 * sr)] = 500
    return pcm


def expected(p, sh, pcm, fft, shift, seg_ends):
    """records and events of the session's own samples, zero-extended to its real frames; the machine starts afresh after every flush"""
    total = seg_ends[-1]
    need = (total - 1) * shift + fft
    x = np.concatenate([pcm, np.zeros(max(0, need - len(pcm)), np.int16)])
    rec = R.run(p["hop"], p["clip_level"], R.frames_of(x, fft, shift)[:total])
    assert len(rec) == total
    ev, t0 = [], 0
    for end in seg_ends:
        mach = R.machine()
        ev += R.events(p, sh, t0, rec[t0:end], mach) + R.flush(p, sh, end, mach)
        t0 = end
    return rec, ev


def host_events(opts, sr, fft, sh, rec, seg_ends):
    """the same through the library's host statement (aprilx_quality_events_host)"""
    plan = A.quality_plan(sr, fft, sh, opts)
    ev, t0 = [], 0
    for end in seg_ends:
        e, _ = A.quality_events_host(plan, sh, t0, rec[t0:end], None, flush=True)
        ev += [x.astuple() for x in e]
        t0 = end
    return ev


FLUSH_MS = 1000                                   # inside the digital silence, and inside the clipping hold of the default options


def mode_live(m, mode, chunking):
    sr, fft, shift, sh = geometry(m)
    assert sr == 16000
    asynchronous = mode == "async"
    pcm, pcm8 = scenario(sr, 5), scenario(8000, 6)
    other = scenario(sr, 7)[::-1].copy()                              # channel 0 of the two-channel stream: something else
    assert len(other) == len(pcm) == 2 * len(pcm8)
    opts = [dict(report_ms=100), dict(clip_level=20000, clip_run_min=1, clip_hold_ms=100, dropout_ms=20, report_ms=370)]
    tel_opts = dict(clip_level=30000, clip_run_min=2, report_ms=200, dropout_ms=50)
    two_opts = dict(report_ms=0, clip_hold_ms=200)
    withq = [Run(m, quality=o, asynchronous=asynchronous) for o in opts]
    twins = [Run(m, asynchronous=asynchronous) for _ in opts]
    tel = Run(m, quality=tel_opts, asynchronous=asynchronous, input_sample_rate=8000, input_format="mulaw")
    two = Run(m, quality=two_opts, asynchronous=asynchronous, input_format="f32", channels=2, channel=1)
    tel_raw = IF.encode(pcm8, "mulaw")
    two_raw = np.stack([other, pcm], axis=1).reshape(-1).astype(np.float32) / np.float32(32768.0)
    two_pcm = A.decode_host(two_raw, ("f32", 2, 1))                   # the samples the session makes of it
    assert len(two_pcm) == len(pcm)
    tel_twin = Run(m, asynchronous=asynchronous, input_sample_rate=8000, input_format="mulaw")
    two_twin = Run(m, asynchronous=asynchronous, input_format="f32", channels=2, channel=1)
    runs, fmt = withq + twins, [tel, two, tel_twin, two_twin]
    grp, fgrp = A.SessionGroup([r.s for r in runs]), A.SessionGroup([r.s for r in fmt])
    before = m.quality_stats()
    books, tel_book = [Book(m.dims) for _ in range(3)], Book(m.dims)
    seg_ends, tel_ends, stream, tel_stream, two_stream = [], [], [], [], []
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
        two_stream += [two_pcm[s0:s1], np.zeros(6400, np.int16)]
        seg16 = np.asarray(m.resample(IF.decode(tel_raw[s0 // 2:s1 // 2], "mulaw"), 8000), np.int16)      # the telephone stream at the model's rate
        tel_book.feed(len(seg16)); tel_book.flush(); tel_ends.append(int(tel_book.frames))
        tel_stream += [seg16, np.zeros(6400, np.int16)]
    stream, tel_stream, two_stream = np.concatenate(stream), np.concatenate(tel_stream), np.concatenate(two_stream)
    out = dict(streams=[], twins=[])
    for a, b in list(zip(withq, twins)) + [(tel, tel_twin), (two, two_twin)]:
        fa, fb = a.s.frames(), b.s.frames()
        out["twins"].append(dict(events=a.ev == b.ev, frames=bool(fa.shape == fb.shape and (fa.view(np.uint32) == fb.view(np.uint32)).all()),
                                 chunks=a.s.chunks() == b.s.chunks(), n_events=len(a.ev), n_chunks=a.s.chunks(), twin_quality=len(b.q),
                                 twin_info=b.s.quality() is None))
    for a, o, x, ends in ((withq[0], opts[0], stream, seg_ends), (withq[1], opts[1], stream, seg_ends), (tel, tel_opts, tel_stream, tel_ends),
                          (two, two_opts, two_stream, seg_ends)):
        p = R.make_plan(sr, fft, sh, R.options(**o))
        rec, want = expected(p, sh, x, fft, shift, ends)
        host = host_events(o, sr, fft, sh, rec, ends)
        info = a.s.quality()
        got = [tuple(g) for g in a.q]
        clipped = int((rec[:, 4] >> 16 >= p["clip_run_min"]).sum())
        out["streams"].append(dict(equal=got == want, host_equal=host == want, got=[list(g) for g in got[:12]], want=[list(w) for w in want[:12]], n_want=len(want),
                                   kinds=sorted(set(w[0] for w in want)), frames_seen=info["frames_seen"], real=ends[-1],
                                   counters=[info["frames"], info["clipped_frames"], info["dead_frames"], info["clip_samples"], info["reports"]],
                                   want_counters=[ends[-1], clipped, int(rec[:, 5].sum()), int((rec[:, 4] & 0xffff).sum()), sum(w[0] == R.REPORT for w in want)],
                                   state=[info["clipping"], info["dropout"]], hop=info["hop"], cku=a.cku,
                                   # the OFF events the first flush gives, at the first segment's end (the silence goes on behind the
                                   # flush: the second segment's DROPOUT_ON carries the same time)
                                   closing=[w[0] for w in want if w[0] in (R.CLIPPING_OFF, R.DROPOUT_OFF) and w[2] == ends[0] * sh]))
    after = m.quality_stats()
    out.update(mismatch=int(m.stats().replay_mismatch), launches=after[0] - before[0], quality_frames=after[1] - before[1],
               want_quality_frames=3 * seg_ends[-1] + tel_ends[-1])
    for r in runs + fmt:
        r.s.close()
    return out


ALL_BURSTS = [(0.15, 0.55), (0.9, 1.35)]          # tone_worker's scenario for all three detectors: two bursts ...
ALL_KEYS = [("7", 0.30), ("#", 0.66)]             # ... a key inside the first, and one between them that the flush falls into
ALL_TONES = [((1100,), 1.45, 0.25), ((480, 620), 1.78, 0.15)]      # ... and two tones behind them
ALL_FLUSH_AT = 0.70


def mode_all4(m):
    """session 0 with voice activity, DTMF, tones AND quality, session 1 with the three detectors only, session 2 with quality only, 3 with
    nothing: one group, the same samples, irregular feeds.  Every detector's events of 0 must be those of 1, the quality events of 0
    those of 2 and of the numpy statement, and nobody's transcript may move"""
    import vad_ref as V
    import dtmf_ref as D
    import tone_ref as T
    sr, fft, shift, sh = geometry(m)
    assert sr == 16000
    sig = V.burst_signal(2.0, ALL_BURSTS, -50.0, 20.0, seed=50).astype(np.int32)
    for d, at in ALL_KEYS:
        tone, onsets = D.digit_signal(d, 100, 0, sr, -200.0, seed=0, tail_ms=0)
        a = int(at * sr)
        sig[a:a + sr // 10] += tone[onsets[0]:onsets[0] + sr // 10]
    for hz, at, dur in ALL_TONES:
        n = int(dur * sr)
        a = int(at * sr)
        sig[a:a + n] += T.to_pcm(T.sine(hz[0], n, sr, -12.0) if len(hz) == 1 else T.pair(hz[0], hz[1], n, sr, -15.0)).astype(np.int32)
    pcm = np.clip(sig, -32768, 32767).astype(np.int16)
    qopt = dict(clip_level=4000, clip_run_min=2, clip_hold_ms=100, dropout_ms=20, report_ms=250)
    runs = [Run(m, quality=q, tones=t, dtmf=t, vad=t) for t, q in ((True, qopt), (True, None), (None, qopt), (None, None))]
    grp = A.SessionGroup([r.s for r in runs])
    s0_ = [m.vad_stats(), m.dtmf_stats(), m.tone_stats(), m.quality_stats()]
    book, seg_ends, stream, single = Book(m.dims), [], [], 0
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
    _, want = expected(R.make_plan(sr, fft, sh, R.options(**qopt)), sh, np.concatenate(stream), fft, shift, seg_ends)
    s1_ = [m.vad_stats(), m.dtmf_stats(), m.tone_stats(), m.quality_stats()]
    out = dict(vad=[[list(e) for e in r.vad] for r in runs], keys=[[list(e) for e in r.keys] for r in runs], tones=[[list(e) for e in r.tones] for r in runs],
               quality=[[list(e) for e in r.q] for r in runs], want_quality=[list(w) for w in want], kinds=sorted(set(w[0] for w in want)),
               single_frame_feeds=single, events=[r.ev == runs[0].ev for r in runs], n_events=len(runs[0].ev), chunks=[r.s.chunks() for r in runs],
               frames=[bool(x.shape == rows[0].shape and (x.view(np.uint32) == rows[0].view(np.uint32)).all()) for x in rows],
               det_frames=[b[1] - a[1] for a, b in zip(s0_, s1_)], launches=[b[0] - a[0] for a, b in zip(s0_, s1_)], real=seg_ends[-1],
               mismatch=int(m.stats().replay_mismatch))
    for r in runs:
        r.s.close()
    return out


def mode_off(m):
    """an engine where nobody opts in (a session with the three detectors only): no quality launch, no quality event; the same feeds
    again with a session that does opt in: the other detectors launch exactly as often; then the rules of aprilx_session_set_quality,
    the refusals of snapshot and restore, and a profiled pass"""
    sr, fft, shift, sh = geometry(m)
    pcm = scenario(sr, 3)
    out = {}

    def det():
        return [m.vad_stats()[0], m.dtmf_stats()[0], m.tone_stats()[0]]

    def feeds(r):
        for a in range(0, len(pcm), sr // 10):
            r.s.feed_pcm16(pcm[a:a + sr // 10])
        r.s.flush()
    d0 = det()
    plain = Run(m, dtmf=True, vad=True, tones=True)
    feeds(plain)
    d1 = det()
    out["unused"] = list(m.quality_stats())
    out["plain_info"] = plain.s.quality()
    out["plain_quality"] = len(plain.q)
    blob = plain.s.snapshot()                                         # (an idle point: the flush has completed)
    plain.s.close()
    opted = Run(m, dtmf=True, vad=True, tones=True, quality=True)
    feeds(opted)
    d2 = det()
    out["others_launches"] = [[b - a for a, b in zip(d0, d1)], [b - a for a, b in zip(d1, d2)]]
    out["used"] = list(m.quality_stats())[:2]
    out["opted_frames"] = opted.s.quality()["frames_seen"]
    out["opted_events"] = len(opted.q)
    opted.s.close()
    L = m._L
    a = Run(m, quality=True)
    out["fresh"] = a.s.quality() is not None

    def raw(size=None, flags=0, handler=True, **kw):
        d = dict(A._QUALITY_DEFAULTS); d.update(kw)
        o = _ffi.AprilxQualityOptions(C.sizeof(_ffi.AprilxQualityOptions) if size is None else size, flags, *[d[n] for n in A._QUALITY_FIELDS])
        return int(L.aprilx_session_set_quality(a.s._handle, C.byref(o), A._QUALITY_HANDLER if handler else C.cast(None, _ffi.QUALITY_HANDLER), id(a.s)))
    out["bad"] = [raw(size=8), raw(flags=2), raw(handler=False), raw(clip_level=1023), raw(clip_level=32768), raw(clip_run_min=0), raw(clip_run_min=65),
                  raw(clip_hold_ms=99), raw(dropout_ms=19), raw(dropout_ms=60001), raw(report_ms=99), raw(report_ms=60001)]
    out["after_bad"] = a.s.quality()["report_frames"]
    out["set"] = raw(report_ms=500, clip_level=32124)
    out["after_set"] = [a.s.quality()["report_frames"], a.s.quality()["clip_level"]]
    half = len(pcm) // 2 // 160 * 160
    a.s.feed_pcm16(pcm[:half])
    out["after_feed"] = raw(report_ms=1000)                           # audio fed since the last completed flush: refused
    out["off_after_feed"] = int(L.aprilx_session_set_quality(a.s._handle, None, C.cast(None, _ffi.QUALITY_HANDLER), None))
    out["still"] = a.s.quality()["report_frames"]
    # snapshot of a session with the observer on, at a point where it would otherwise be taken (idle, between feeds)
    a.s.drain()
    out["snapshot_refused"] = int(L.aprilx_session_snapshot(a.s._handle, None, 0))
    a.s.feed_pcm16(pcm[half:]); a.s.flush()
    info = a.s.quality()
    out["frames_seen"] = info["frames_seen"]
    out["counters"] = [info["frames"], info["reports"], info["dead_frames"]]
    out["report_times"] = [e[2] for e in a.q if e[0] == R.REPORT][:4]
    out["after_flush"] = raw()
    # restore into a session with the observer on is refused with a message; into the same session with it off it is taken
    b = Run(m, dtmf=True, vad=True, tones=True, quality=True)
    try:
        b.s.restore(blob)
        out["restore_refused"] = None
    except ValueError as e:
        out["restore_refused"] = str(e)
    b.s.set_quality(None)
    b.s.restore(blob)
    out["restore_taken"] = True
    a.s.set_quality(None)
    out["off"] = a.s.quality()
    out["snapshot_when_off"] = int(L.aprilx_session_snapshot(a.s._handle, None, 0)) > 0
    before = list(m.quality_stats())[:2]
    n_ev = len(a.q)
    a.s.feed_pcm16(pcm); a.s.flush()
    out["off_launches_nothing"] = list(m.quality_stats())[:2] == before and len(a.q) == n_ev
    m.profile(1)
    c = Run(m, quality=True)
    c.s.feed_pcm16(pcm); c.s.flush()
    m.profile(0)
    out["profiled_ms"] = m.quality_stats()[2]
    out["profiled_kinds"] = sorted(set(e[0] for e in c.q))
    out["mismatch"] = int(m.stats().replay_mismatch)
    return out


def main():
    path, mode = sys.argv[1], sys.argv[2]
    m = A.Model(path)
    if mode == "kernel":
        res = mode_kernel(m)
    elif mode == "live":
        res = {c: mode_live(m, sys.argv[3], c) for c in sys.argv[4:]}
    elif mode == "all4":
        res = mode_all4(m)
    else:
        res = mode_off(m)
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
