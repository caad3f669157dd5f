"""Worker for tests/test_gpu_dtmf.py: DTMF digits per session (aprilx_session_set_dtmf), beside voice activity in the same passes
(mode "both"), and the kernel alone (aprilx_run_dtmf, aprilx_run_dtmf_decide), one scenario per process.  Prints one line "RESULT <json>".
usage: dtmf_worker.py model.april mode [args ...]

What the detector must give comes from the numpy statement of the contract (tests/dtmf_ref.py), never from the product; only the
tables are the library's (checked against numpy's on the CPU), so that libm differences cannot leak in."""
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
import dtmf_ref as R  # noqa: E402
import input_format_ref as IF  # noqa: E402
from vad_worker import Book, cuts, shift_ms_of  # noqa: E402
from vad_worker import expected as vad_expected  # noqa: E402

N_SET = (1, 3, 4, 5, 63, 64, 65, 257)            # around a workgroup's four waves, its 16 frames, and the frames one pass of 64 workgroups walks


def plan_dict(p):
    return dict(Wd=p.Wd, half_w=R.F(p.half_w), min_power=R.F(p.min_power), twist_hi=R.F(p.twist_hi), twist_lo=R.F(p.twist_lo), rel_peak=R.F(p.rel_peak),
                min_share=R.F(p.min_share), on_frames=p.on_frames, off_frames=p.off_frames)


def geometry(m):
    return int(m.dims.sample_rate), int(m.dims.fft_size), int(m.dims.frame_shift), shift_ms_of(m)


def same_bits(a, b):
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def frame_pool(sr, fft, shift):
    """frames of the digit string at two noise levels, then silence, the lowest sample throughout, and random edge samples"""
    rng = np.random.RandomState(11)
    a, _ = R.digit_signal(R.STRING, 40, 40, sr, -50.0, 0, seed=1)
    b, _ = R.digit_signal(R.STRING[::-1], 45, 45, sr, -30.0, shift // 3, seed=2, level_dbfs=-20.0)
    edge = np.stack([np.zeros(fft, np.int16), np.full(fft, -32768, np.int16), rng.choice(np.array([-32768, 32767, 0, 1, -1], np.int16), size=fft)])
    return np.concatenate([R.frames_of(a, fft, shift), edge, R.frames_of(b, fft, shift)])


def mode_kernel(m):
    sr, fft, shift, sh = geometry(m)
    plan = A.dtmf_plan(sr, fft, sh)
    p, tab = plan_dict(plan), A.dtmf_tables(sr, plan.Wd)
    pool = frame_pool(sr, fft, shift)
    bad, calls, tones = [], 0, 0
    for n in N_SET:
        off = 9 if n < 60 else 0                                  # (short runs start where the first digit does)
        fr = pool[off:off + n]
        assert len(fr) == n
        want_c, want_p = R.run(p, tab, fr)
        codes, pw = m.run_dtmf([True], [fr])
        calls += 1
        if codes[0].tolist() != want_c.tolist() or not same_bits(pw[0], want_p):
            bad.append(["n%d" % n, int((codes[0] != want_c).sum()), int((pw[0].view(np.uint32) != want_p.view(np.uint32)).sum())])
        tones += int((want_c != 0).sum())
    # four runs with different options in ONE launch
    opts = [True, dict(min_level_dbfs=-10.0), dict(twist_hi_db=0.0, twist_lo_db=0.0, rel_peak_db=30.0), dict(min_share=1.0, min_level_dbfs=-70.0)]
    lens, offs = (65, 5, 257, 1), (0, 9, 20, 12)
    frs = [pool[o:o + n] for n, o in zip(lens, offs)]
    codes, pw = m.run_dtmf(opts, frs)
    calls += 1
    differ = 0
    for r in range(4):
        pr = plan_dict(A.dtmf_plan(sr, fft, sh, opts[r]))
        want_c, want_p = R.run(pr, tab, frs[r])
        if codes[r].tolist() != want_c.tolist() or not same_bits(pw[r], want_p):
            bad.append(["multi%d" % r, int((codes[r] != want_c).sum()), int((pw[r].view(np.uint32) != want_p.view(np.uint32)).sum())])
        differ += int(want_c.tolist() != R.run(p, tab, frs[r])[0].tolist())
    # the decision alone on the tie rows (and on the pool's own powers)
    ties = R.tie_rows(p)
    got = m.run_dtmf_decide(True, np.stack([q for q, _ in ties]))
    tie_bad = [i for i, (_, code) in enumerate(ties) if int(got[i]) != code]
    _, pool_p = R.run(p, tab, pool[:80])
    calls += 2
    if m.run_dtmf_decide(True, pool_p).tolist() != [R.decide(p, q) for q in pool_p]:
        bad.append(["decide_pool"])
    # refusals of aprilx_run_dtmf
    L = m._L
    o1 = (_ffi.AprilxDtmfOptions * 1)(A._dtmf_options(True))
    n1 = np.array([2], np.int32); fr = np.zeros((2, fft), np.int16); by = np.zeros(2, np.uint8)

    def call(n_runs=1, n=2, size=None):
        n1[0] = n
        o1[0].size = C.sizeof(_ffi.AprilxDtmfOptions) if size is None else size
        return int(L.aprilx_run_dtmf(m._handle, C.addressof(o1), n_runs, n1.ctypes.data, fr.ctypes.data, by.ctypes.data, None))
    refusals = [call(n_runs=0), call(n=0), call(n=-1), call(size=8), call()]
    return dict(bad=bad, calls=calls, tones=tones, tie_bad=tie_bad, n_ties=len(ties), differ=differ, refusals=refusals, Wd=plan.Wd)


class Run:
    """one session's callbacks (type, token text, logprob bits, flags, time) and its DTMF events, in delivery order"""

    def __init__(self, m, dtmf=None, asynchronous=False, **kw):
        self.ev, self.keys, self.cku = [], [], 0

        def h(t, toks):
            if int(t) == 3:
                self.cku += 1
            self.ev.append((int(t), [(x[0], struct.pack("<f", float(x[1])), int(x[2]), int(x[3])) for x in toks]))
        self.s = A.Session(m, h, raw_events=True, asynchronous=asynchronous, no_rt=asynchronous, dtmf=dtmf,
                           dtmf_callback=lambda e: self.keys.append((e.kind, e.digit, e.time_ms)), **kw)


HELD_MS = 200                                     # the key the first flush falls into
ITEMS1 = [(None, 100)] + [x for d in R.STRING[:12] for x in ((d, 40), (None, 40))]
ITEMS2 = [(None, 40)] + [x for d in R.STRING[12:] for x in ((d, 45), (None, 45))] + [(None, 200)]
ITEMS = ITEMS1 + [("9", HELD_MS)] + ITEMS2
FLUSH_MS = sum(ms for _, ms in ITEMS1) + HELD_MS // 2
WANT_DIGITS = R.STRING[:12] + "99" + R.STRING[12:]              # (the flush splits the held 9 into two keys)


def expected(p, tab, sh, pcm, fft, shift, seg_ends):
    """codes and events of the session's own samples, zero-extended to its real frames; the machine starts afresh after every flush"""
    total = seg_ends[-1]
    need = (total - 1) * shift + fft
    x = np.concatenate([pcm, np.zeros(max(0, need - len(pcm)), np.int16)])
    codes, _ = R.run(p, tab, R.frames_of(x, fft, shift)[:total])
    assert len(codes) == total
    ev, t0 = [], 0
    for end in seg_ends:
        mach = R.machine()
        ev += R.events(p, sh, t0, codes[t0:end], mach) + R.flush(sh, end, mach)
        t0 = end
    return codes, ev


def mode_live(m, mode, chunking):
    sr, fft, shift, sh = geometry(m)
    assert sr == 16000
    asynchronous = mode == "async"
    pcm, _ = R.keys_signal(ITEMS, sr, -50.0, seed=5)
    pcm8, _ = R.keys_signal(ITEMS, 8000, -50.0, seed=6)
    other = R.keys_signal([(None, 60)] + [x for d in "8#2*" * 14 for x in ((d, 30), (None, 20))] + [(None, 1000)], sr, -45.0, seed=7)[0][:len(pcm)]
    assert len(other) == len(pcm) == 2 * len(pcm8)
    # (the second stream takes only keys of 60 ms or more -- the 200 ms one the flush falls into --, and its pause of 600 ms outlasts the
    # 400 ms of zeros a flush appends: it still holds that key when the flush completes)
    opts = [True, dict(min_tone_ms=60, min_pause_ms=600)]
    plans = [A.dtmf_plan(sr, fft, sh, o) for o in opts]
    tab = A.dtmf_tables(sr, plans[0].Wd)
    withd = [Run(m, dtmf=o, asynchronous=asynchronous) for o in opts]
    twins = [Run(m, asynchronous=asynchronous) for _ in opts]
    tel = Run(m, dtmf=True, asynchronous=asynchronous, input_sample_rate=8000, input_format="mulaw")
    two = Run(m, dtmf=True, asynchronous=asynchronous, input_format="s16", channels=2, channel=1)
    tel_raw = IF.encode(pcm8, "mulaw")
    two_raw = np.stack([other, pcm], axis=1).reshape(-1).astype("<i2")
    # ... and their twins without the detector, in the same group, fed the same bytes
    tel_twin = Run(m, asynchronous=asynchronous, input_sample_rate=8000, input_format="mulaw")
    two_twin = Run(m, asynchronous=asynchronous, input_format="s16", channels=2, channel=1)
    runs, fmt = withd + twins, [tel, two, tel_twin, two_twin]
    grp, fgrp = A.SessionGroup([r.s for r in runs]), A.SessionGroup([r.s for r in fmt])
    before = m.dtmf_stats()
    books, tel_book = [Book(m.dims) for _ in range(3)], Book(m.dims)      # the two PCM16 streams and the two-channel one; the telephone one
    seg_ends, tel_ends, stream = [], [], []
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
        tel_book.feed(len(m.resample(pcm8[s0 // 2:s1 // 2], 8000))); tel_book.flush(); tel_ends.append(int(tel_book.frames))
    stream = np.concatenate(stream)
    out = dict(streams=[], twins=[], formatted=[])
    for a, b in list(zip(withd, twins)) + [(tel, tel_twin), (two, two_twin)]:      # (the test reads twins[2:] as the formatted ones)
        fa, fb = a.s.frames(), b.s.frames()
        out["twins"].append(dict(events=a.ev == b.ev, frames=bool(fa.shape == fb.shape and (fa.view(np.uint32) == fb.view(np.uint32)).all()),
                                 chunks=a.s.chunks() == b.s.chunks(), n_events=len(a.ev), n_chunks=a.s.chunks(), twin_keys=len(b.keys),
                                 twin_info=b.s.dtmf_info() is None))
    for a, plan in zip(withd, plans):
        p = plan_dict(plan)
        codes, want = expected(p, tab, sh, stream, fft, shift, seg_ends)
        info = a.s.dtmf_info()
        out["streams"].append(dict(equal=a.keys == want, got=a.keys[:60], want=want[:60], digits=R.digits_of(a.keys), n_want=len(want),
                                   frames_seen=info["frames_seen"], real=seg_ends[-1], tone_frames=info["tone_frames"], want_tone=int((codes != 0).sum()),
                                   info_digits=info["digits"], held=info["held"], Wd=info["Wd"], off_frames=info["off_frames"], cku=a.cku,
                                   # the flush inside the held key: an UP exactly at the first segment's end
                                   closing=(R.UP, "9", seg_ends[0] * sh) in a.keys))
    ref = withd[0].keys
    for a, ends in ((tel, tel_ends), (two, seg_ends)):
        info = a.s.dtmf_info()
        same_len = len(a.keys) == len(ref)
        worst = max([abs(g[2] - w[2]) for g, w in zip(a.keys, ref)] or [0])
        out["formatted"].append(dict(digits=R.digits_of(a.keys), kinds=same_len and [(g[0], g[1]) for g in a.keys] == [(w[0], w[1]) for w in ref],
                                     worst_ms=int(worst), frames_seen=info["frames_seen"], real=ends[-1], cku=a.cku, got=a.keys[:60]))
    after = m.dtmf_stats()
    out.update(mismatch=int(m.stats().replay_mismatch), launches=after[0] - before[0], dtmf_frames=after[1] - before[1],
               want_dtmf_frames=3 * seg_ends[-1] + tel_ends[-1], on_ms=plans[0].on_frames * sh, want_digits=WANT_DIGITS)
    for r in runs + fmt:
        r.s.close()
    return out


def mode_rules(m):
    sr, fft, shift, sh = geometry(m)
    pcm, _ = R.keys_signal([(None, 100)] + [x for d in "159D" for x in ((d, 60), (None, 60))] + [(None, 300)], sr, -50.0, seed=3)
    out = {}
    plain = Run(m)
    plain.s.feed_pcm16(pcm); plain.s.flush()
    out["unused"] = list(m.dtmf_stats())                         # no session has opted in: nothing was launched
    out["plain_info"] = plain.s.dtmf_info()
    L = m._L
    a = Run(m, dtmf=True)
    out["fresh"] = a.s.dtmf_info() is not None

    def raw(size=None, flags=0, handler=True, **kw):
        d = dict(A._DTMF_DEFAULTS); d.update(kw)
        o = _ffi.AprilxDtmfOptions(C.sizeof(_ffi.AprilxDtmfOptions) if size is None else size, d["min_level_dbfs"], d["twist_hi_db"], d["twist_lo_db"],
                                   d["rel_peak_db"], d["min_share"], d["min_tone_ms"], d["min_pause_ms"], flags)
        return int(L.aprilx_session_set_dtmf(a.s._handle, C.byref(o), A._DTMF_HANDLER if handler else C.cast(None, _ffi.DTMF_HANDLER), id(a.s)))
    out["bad"] = [raw(size=8), raw(flags=2), raw(handler=False), raw(min_level_dbfs=1.0), raw(twist_hi_db=-1.0), raw(twist_lo_db=21.0), raw(rel_peak_db=2.0),
                  raw(min_share=0.0), raw(min_tone_ms=5), raw(min_pause_ms=2000), raw(min_share=float("nan"))]
    out["after_bad"] = a.s.dtmf_info()["on_frames"]              # nothing changed
    out["set"] = raw(min_tone_ms=40)
    out["after_set"] = a.s.dtmf_info()["on_frames"]
    half = len(pcm) // 2
    a.s.feed_pcm16(pcm[:half])
    out["after_feed"] = raw(min_tone_ms=20)                       # audio fed since the last completed flush: refused
    out["off_after_feed"] = int(L.aprilx_session_set_dtmf(a.s._handle, None, C.cast(None, _ffi.DTMF_HANDLER), None))
    out["still"] = a.s.dtmf_info()["on_frames"]
    a.s.feed_pcm16(pcm[half:]); a.s.flush()
    out["used"] = list(m.dtmf_stats())[:2]
    info = a.s.dtmf_info()
    out["frames_seen"] = info["frames_seen"]
    out["digits_found"] = [R.digits_of(a.keys), info["digits"], info["tone_frames"]]
    out["after_flush"] = raw(min_tone_ms=20)
    info = a.s.dtmf_info()
    out["counters_restart"] = [info["digits"], info["tone_frames"], info["frames_seen"], info["on_frames"]]
    a.s.set_dtmf(None)
    out["off"] = a.s.dtmf_info()
    before = list(m.dtmf_stats())[:2]
    n_keys = len(a.keys)
    a.s.feed_pcm16(pcm); a.s.flush()
    out["off_launches_nothing"] = list(m.dtmf_stats())[:2] == before and len(a.keys) == n_keys
    # a profiled pass accounts the kernel's time
    m.profile(1)
    b = Run(m, dtmf=True)
    b.s.feed_pcm16(pcm); b.s.flush()
    m.profile(0)
    out["profiled_ms"] = m.dtmf_stats()[2]
    out["profiled_digits"] = R.digits_of(b.keys)
    out["mismatch"] = int(m.stats().replay_mismatch)
    return out


BOTH_BURSTS = [(0.15, 0.55), (0.9, 1.35)]        # two of vad_worker's bursts in 1.5 s ...
BOTH_KEYS = [("7", 0.30), ("#", 0.66)]            # ... a key of 100 ms inside the first, and one between them that the flush falls into
BOTH_FLUSH_AT = 0.70


def mode_both(m):
    """both detectors in the same passes: session 0 with VAD and DTMF, 1 with VAD, 2 with DTMF, 3 with neither, one group, the same samples.
    A pass's DTMF bytes then sit behind its VAD bytes, and session 0's runs are at different offsets in the two parts"""
    import vad_ref as V
    sr, fft, shift, sh = geometry(m)
    assert sr == 16000
    _, mel = m.fbank_tables()
    sig = V.burst_signal(1.5, BOTH_BURSTS, -50.0, 20.0, seed=50).astype(np.int32)
    for d, at in BOTH_KEYS:
        tone, onsets = R.digit_signal(d, 100, 0, sr, -200.0, seed=0, tail_ms=0)      # (the digit alone: noise far below one int16 step)
        a = int(at * sr)
        sig[a:a + sr // 10] += tone[onsets[0]:onsets[0] + sr // 10]
    pcm = np.clip(sig, -32768, 32767).astype(np.int16)
    vplan = V.make_plan(mel, sr, sh, V.options())
    dplan = A.dtmf_plan(sr, fft, sh)
    p, tab = plan_dict(dplan), A.dtmf_tables(sr, dplan.Wd)
    runs = []
    for vad, dtmf in ((True, True), (True, None), (None, True), (None, None)):
        got = []
        runs.append(Run(m, dtmf=dtmf, vad=vad, vad_callback=lambda e, got=got: got.append((e.kind, e.time_ms))))
        runs[-1].vad = got
    grp = A.SessionGroup([r.s for r in runs])
    v0, d0 = m.vad_stats(), m.dtmf_stats()
    book, seg_ends, stream, single = Book(m.dims), [], [], 0
    cut_at = int(BOTH_FLUSH_AT * sr)
    for si, (s0, s1) in enumerate([(0, cut_at), (cut_at, len(pcm))]):
        bounds = cuts(s1 - s0, "irregular", sr // 10, seed=25 + si)      # (seeds whose cuts hold single-frame feeds in both segments)
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
    _, want_keys = expected(p, tab, sh, np.concatenate(stream), fft, shift, seg_ends)
    v1, d1 = m.vad_stats(), m.dtmf_stats()
    out = dict(vad=[r.vad for r in runs], keys=[r.keys for r in runs], want_vad=want_vad, want_keys=want_keys, single_frame_feeds=single,
               events=[r.ev == runs[0].ev for r in runs], n_events=len(runs[0].ev), chunks=[r.s.chunks() for r in runs],
               frames=[bool(x.shape == rows[0].shape and (x.view(np.uint32) == rows[0].view(np.uint32)).all()) for x in rows],
               vad_frames=v1[1] - v0[1], dtmf_frames=d1[1] - d0[1], real=seg_ends[-1], launches=[v1[0] - v0[0], d1[0] - d0[0]],
               mismatch=int(m.stats().replay_mismatch))
    for r in runs:
        r.s.close()
    return out


def main():
    path, mode = sys.argv[1], sys.argv[2]
    m = A.Model(path)
    if mode == "kernel":
        res = mode_kernel(m)
    elif mode == "live":
        res = {c: mode_live(m, sys.argv[3], c) for c in sys.argv[4:]}
    elif mode == "both":
        res = mode_both(m)
    else:
        res = mode_rules(m)
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
