"""Worker for tests/test_gpu_vad.py: voice activity per session (aprilx_session_set_vad) and the kernel alone (aprilx_run_vad), one
scenario per process.  Prints one line "RESULT <json>".
usage: vad_worker.py model.april mode [args ...]

What the detector must give comes from the numpy statement of the contract (tests/vad_ref.py), never from the product."""
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
import vad_ref as R  # noqa: E402
import input_format_ref as IF  # noqa: E402

NB_SET = (1, 15, 16, 17, 54, 80)
N_SET = (1, 15, 16, 17, 255, 256, 257, 300)
PAD = np.float32(np.log(np.float64(1.1920928955078125e-07)))


def shift_ms_of(m):
    return int(m.dims.frame_shift) * 1000 // int(m.dims.sample_rate)


def band_options(mel, rate, shift_ms, nb, seed=0, **kw):
    """options whose band holds exactly nb bins of this mel table (the limits sit on bin peaks), and their reference plan"""
    peaks = np.argmax(mel, axis=1).astype(np.float64) * rate / (2.0 * mel.shape[1])
    starts = list(range(len(peaks) - nb + 1))
    np.random.RandomState(seed).shuffle(starts)
    for b0 in starts:
        lo, hi = float(peaks[b0]), float(peaks[b0 + nb - 1])
        if not lo < hi:
            hi = lo + 1.0
        o = R.options(band_lo_hz=lo, band_hi_hz=hi, **kw)
        p = R.make_plan(mel, rate, shift_ms, o)
        if p is not None and p["b1"] - p["b0"] == nb:
            return o, p
    raise RuntimeError("no band of %d bins" % nb)


def rows_for(plan, n, rng, ties):
    """rows that move the state machine: quiet and loud stretches, pad-value rows, -0.0; with `ties` (bands of 1 or 16 bins, where the
    band mean of a constant row is the constant) frames whose d equals a threshold exactly"""
    nbins = 80
    level = np.repeat(rng.choice([-14.0, -9.0, -5.0, 0.0], size=(n + 19) // 20), 20)[:n]
    x = (level[:, None] + rng.normal(0, 1.5, size=(n, nbins))).astype(np.float32)
    x[rng.rand(n) < 0.05] = PAD
    x[rng.rand(n, nbins) < 0.01] = np.float32(-0.0)
    if ties and n >= 6:
        # s = 0 on the first frame; then e = 4 thr_on: t = 4 thr_on, 0.25 t = thr_on, s = thr_on, d = thr_on exactly: not above it
        x[0] = 0.0
        x[1] = np.float32(4.0) * plan["thr_on"]
        x[2] = x[1]
    return x


def check(name, got, want, bad):
    gb, ge, gs = got
    wb, we, wv = want
    ok = gb.tolist() == wb.tolist() and (ge.view(np.uint32) == we.view(np.uint32)).all() and state_of(gs) == R.state_tuple(wv)
    if not ok:
        bad.append([name, int((gb != wb).sum()), int((ge.view(np.uint32) != we.view(np.uint32)).sum()), state_of(gs) == R.state_tuple(wv)])
    return ok


def state_of(st):
    fl = np.array([st.s, st.cur] + list(st.hist), np.float32).view(np.uint32).tolist()
    return tuple(fl) + (st.cnt, st.pos, st.st, st.run, st.first)


def copy_state(st):
    return _ffi.AprilxVadState.from_buffer_copy(bytes(st))


def mode_kernel(m):
    sr, sh = int(m.dims.sample_rate), shift_ms_of(m)
    _, mel = m.fbank_tables()
    bad, calls, tie_frames, speech_runs = [], 0, 0, 0
    # every band width x every length, one run per launch
    for nb in NB_SET:
        for n in N_SET:
            rng = np.random.RandomState(1000 * nb + n)
            o, plan = band_options(mel, sr, sh, nb, seed=n)
            rows = rows_for(plan, n, rng, ties=nb in (1, 16))
            want = R.run(plan, rows)
            b, e, st = m.run_vad([o], [rows])
            calls += 1
            check("nb%d_n%d" % (nb, n), (b[0], e[0], st[0]), want, bad)
            if nb in (1, 16) and n >= 6:
                tie_frames += int(want[1][1] == np.float32(4.0) * plan["thr_on"] and want[0][1] == 0)
            speech_runs += int((want[0] & 1).any())
    # eight runs with different options and lengths in ONE launch; runs 1 and 5 wrap their scratch ring (300 rows)
    rng = np.random.RandomState(5)
    opts, plans, rows_l, first = [], [], [], []
    for r, (nb, n) in enumerate(zip((80, 54, 17, 16, 15, 1, 54, 80), (300, 257, 256, 255, 17, 16, 15, 1))):
        o, plan = band_options(mel, sr, sh, nb, seed=r, onset_db=4.0 + r, offset_db=1.0 + 0.5 * r, onset_ms=10 + 10 * r, hangover_ms=50 * (r + 1),
                               min_energy=-13.0 + r)
        opts.append(o); plans.append(plan); rows_l.append(rows_for(plan, n, rng, ties=False))
        first.append({1: 200, 5: 295}.get(r, 0 if r % 2 == 0 else 7))
    b, e, st = m.run_vad(opts, rows_l, first_row=first)
    calls += 1
    states = []
    for r in range(8):
        want = R.run(plans[r], rows_l[r])
        check("multi%d" % r, (b[r], e[r], st[r]), want, bad)
        states.append(want[2])
    # ... and their states carried into a second launch with new rows
    rows2 = [rows_for(plans[r], n, rng, ties=False) for r, n in enumerate((33, 300, 1, 64, 100, 257, 31, 32))]
    b2, e2, st2 = m.run_vad(opts, rows2, first_row=[299, 0, 3, 250, 299, 100, 0, 280], states=[copy_state(x) for x in st])
    calls += 1
    for r in range(8):
        want = R.run(plans[r], rows2[r], states[r])
        check("carried%d" % r, (b2[r], e2[r], st2[r]), want, bad)
    # refusals of aprilx_run_vad
    L = m._L
    o1 = (_ffi.AprilxVadOptions * 1)(A._vad_options(True))
    n1 = np.array([4], np.int32); f1 = np.array([0], np.int32); rows = np.zeros((4, 80), np.float32)
    s1 = (_ffi.AprilxVadState * 1)(A.vad_reset_state()); by = np.zeros(4, np.uint8)

    def call(n_runs=1, first_row=0, size=None):
        f1[0] = first_row
        o1[0].size = C.sizeof(_ffi.AprilxVadOptions) if size is None else size
        return int(L.aprilx_run_vad(m._handle, n_runs, C.addressof(o1), n1.ctypes.data, f1.ctypes.data, rows.ctypes.data, C.addressof(s1), by.ctypes.data, None))
    refusals = [call(n_runs=0), call(first_row=4), call(first_row=-1), call(size=8), call()]
    return dict(bad=bad, calls=calls, tie_frames=tie_frames, speech_runs=speech_runs, refusals=refusals)


class Run:
    """one session's callbacks (type, token text, logprob bits, flags, time) and its voice-activity events, in delivery order"""

    def __init__(self, m, vad=None, asynchronous=False, **kw):
        self.ev, self.vad, self.cku = [], [], 0

        def h(t, toks):
            if int(t) == 3:
                self.cku += 1
            self.ev.append((int(t), [(x[0], struct.pack("<f", float(x[1])), int(x[2]), int(x[3])) for x in toks]))
        self.s = A.Session(m, h, raw_events=True, asynchronous=asynchronous, no_rt=asynchronous, vad=vad,
                           vad_callback=lambda e: self.vad.append((e.kind, e.time_ms)), **kw)


def cuts(n, chunking, unit, seed):
    if chunking == "whole":
        return [0, n]
    if chunking == "100ms":
        return list(range(0, n, unit)) + [n]
    rng = np.random.RandomState(seed)
    sizes = [1, 1, 2, 7, 159, 160, 161, unit // 2, unit, unit, 3 * unit, 5 * unit + 3]      # (160 samples: a single-frame feed)
    at, out = 0, [0]
    while at < n:
        at = min(n, at + int(rng.choice(sizes)))
        out.append(at)
    return out


class Book:
    """Which rows of a session's feature ring are real frames: the bookkeeping of the reference's online filterbank, restated.  Frame k
    covers stream samples [k shift, k shift + padded); a flush drains with padding rows (never real frames), appends 6400 zeros whose
    frames are real, and drains again."""

    def __init__(self, d):
        self.shift, self.padded, self.seg, self.step = int(d.frame_shift), int(d.fft_size), int(d.seg), int(d.seg_step)
        self.n = 0              # stream samples so far
        self.frames = 0         # real frames so far
        self.av = self.sh = 0
        self.real = []          # per ring row: real or padding

    def _cut(self):
        k = max(0, (self.n - self.padded) // self.shift + 1) - self.frames if self.n >= self.padded else 0
        if k > 0:
            self.frames += k; self.real += [True] * k
            self.av += k; self.sh = self.av
        while self.av >= self.seg:
            self.av -= self.step; self.sh -= self.step

    def _drain(self):
        while self.sh >= -3 * self.seg:
            need = max(0, self.seg - self.av)
            self.real += [False] * need
            self.av += need
            self.av -= self.step; self.sh -= self.step

    def feed(self, samples):
        self.n += samples
        self._cut()

    def flush(self):
        self._drain()
        self.feed(6400)
        self._drain()


def expected(plan, shift_ms, rows, segments_end):
    """events of the session's real rows: the detector starts afresh after every completed flush (segments_end: real-frame counts)"""
    ev, bytes_all, t0 = [], [], 0
    for end in segments_end:
        b, _, _ = R.run(plan, rows[t0:end])
        e, last = R.events(plan, shift_ms, t0, b, 0)
        ev += e + R.flush_end(end, shift_ms, last)
        bytes_all.append(b)
        t0 = end
    return ev, np.concatenate(bytes_all)


BURSTS = [(0.8, 1.5), (2.3, 3.0), (3.9, 4.5), (5.3, 6.0), (6.9, 8.1), (9.0, 9.5)]
STREAMS = [(-50.0, 20.0), (-60.0, 30.0), (-40.0, 10.0)]            # (noise dBFS, SNR dB)
FLUSH_AT = 7.4                                                    # inside the fifth burst


def mode_live(m, mode, chunking):
    sr, sh = int(m.dims.sample_rate), shift_ms_of(m)
    _, mel = m.fbank_tables()
    asynchronous = mode == "async"
    # (a hangover of 600 ms outlasts the 400 ms of zeros a flush appends: those streams are still in speech when the flush completes)
    opts = [dict(hangover_ms=600), dict(onset_db=6.0, offset_db=2.5, onset_ms=30, hangover_ms=200), dict(band_lo_hz=300.0, band_hi_hz=3400.0, min_energy=-13.0)]
    plans = [R.make_plan(mel, sr, sh, R.options(**(o if isinstance(o, dict) else {}))) for o in opts]
    pcms = [R.burst_signal(10.0, BURSTS, nd, snr, seed=30 + i) for i, (nd, snr) in enumerate(STREAMS)]
    withv = [Run(m, vad=o, asynchronous=asynchronous) for o in opts]
    twins = [Run(m, asynchronous=asynchronous) for _ in opts]
    # a telephone stream: mu-law at 8000 Hz, the same detector behind the decode and the resampler
    tel_pcm = R.burst_signal(10.0, BURSTS, -50.0, 20.0, seed=40, rate=8000)
    tel_raw = IF.encode(tel_pcm, "mulaw")
    tel = Run(m, vad=dict(band_hi_hz=3400.0, hangover_ms=600), asynchronous=asynchronous, input_sample_rate=8000, input_format="mulaw")
    tel_plan = R.make_plan(mel, sr, sh, R.options(band_hi_hz=3400.0, hangover_ms=600))
    runs = withv + twins
    grp, tel_grp = A.SessionGroup([r.s for r in runs]), A.SessionGroup([tel.s])
    books = [Book(m.dims) for _ in withv]
    tel_book = Book(m.dims)
    seg_ends, tel_seg_ends = [[] for _ in withv], []
    cut_at = int(FLUSH_AT * sr)
    for si, (s0, s1) in enumerate([(0, cut_at), (cut_at, 10 * sr)]):
        bounds = cuts(s1 - s0, chunking, sr // 10, seed=si)
        if asynchronous and chunking == "whole":            # (an asynchronous session refuses a feed of 3 s or more: CANT_KEEP_UP)
            bounds = list(range(0, s1 - s0, 2 * sr)) + [s1 - s0]
        for k, (f0, f1) in enumerate(zip(bounds[:-1], bounds[1:])):
            bufs = [pcms[i % 3][s0 + f0:s0 + f1] for i in range(6)]
            tbuf = tel_raw[(s0 + f0) // 2:(s0 + f1) // 2]
            if mode == "sync":
                grp.feed(bufs); tel_grp.feed_bytes([tbuf])
            elif mode == "pipe2":
                grp.feed_pipelined(bufs, 2); tel_grp.feed_bytes([tbuf], 2)
            else:
                for r, b in zip(runs, bufs):
                    r.s.feed_pcm16(b)
                tel.s.feed(tbuf)
                if chunking == "whole" or k % 8 == 7:       # (keeps the ingest queues below that bound)
                    grp.drain(); tel_grp.drain()
        grp.flush(); tel_grp.flush()
        grp.drain(); tel_grp.drain()
        for i, bk in enumerate(books):
            bk.feed(s1 - s0); bk.flush(); seg_ends[i].append(bk.frames)
        tel_book.feed(len(m.resample(tel_pcm[s0 // 2:s1 // 2], 8000))); tel_book.flush(); tel_seg_ends.append(tel_book.frames)
    out = dict(streams=[], twins=[])
    for i, (a, b) in enumerate(zip(withv, twins)):
        fa, fb = a.s.frames(), b.s.frames()
        out["twins"].append(dict(events=a.ev == b.ev, frames=bool(fa.shape == fb.shape and (fa.view(np.uint32) == fb.view(np.uint32)).all()),
                                 chunks=a.s.chunks() == b.s.chunks(), tokens=sum(len(t) for _, t in a.ev), n_chunks=a.s.chunks(), twin_vad=len(b.vad)))
    for a, bk, plan, ends in list(zip(withv, books, plans, seg_ends)) + [(tel, tel_book, tel_plan, tel_seg_ends)]:
        rows = a.s.frames()
        if len(rows) != len(bk.real):
            raise RuntimeError("the test's frame bookkeeping gives %d ring rows, the session wrote %d" % (len(bk.real), len(rows)))
        real = rows[np.array(bk.real)]
        want, want_bytes = expected(plan, sh, real, ends)
        info = a.s.vad_info()
        out["streams"].append(dict(equal=a.vad == want, got=a.vad[:40], want=want[:40], segments=sum(1 for k, _ in want if k == R.START),
                                   frames_seen=info["frames_seen"], real=int(bk.frames), info_segments=info["segments"],
                                   speech_frames=info["speech_frames"], want_speech=int((want_bytes & 1).sum()), in_speech=info["in_speech"],
                                   long_hangover=plan["hangover_frames"] == 600 // sh,
                                   band=[info["b0"], info["b1"]], want_band=[plan["b0"], plan["b1"]], cku=a.cku,
                                   # the flush in mid-speech: a SPEECH_END exactly at the first segment's end, and speech found after it
                                   closing=(R.END, ends[0] * sh) in a.vad, after=sum(1 for k, t in a.vad if k == R.START and t >= ends[0] * sh)))
    st = m.stats()
    launches, frames, _ = m.vad_stats()
    out.update(mismatch=int(st.replay_mismatch), launches=launches, vad_frames=frames,
               want_vad_frames=sum(int(b.frames) for b in books) + int(tel_book.frames))
    for r in runs + [tel]:
        r.s.close()
    return out


def mode_rules(m):
    sr = int(m.dims.sample_rate)
    pcm = R.burst_signal(2.0, [(0.5, 1.2)], seed=3)
    out = {}
    plain = Run(m)
    plain.s.feed_pcm16(pcm); plain.s.flush()
    out["unused"] = list(m.vad_stats())                          # no session has opted in: nothing was launched
    out["plain_info"] = plain.s.vad_info()
    out["plain_frames_seen"] = plain.s.frames_seen()
    L = m._L
    a = Run(m, vad=True)
    out["fresh"] = a.s.vad_info() is not None

    def raw(size=None, flags=0, handler=True, **kw):
        d = dict(A._VAD_DEFAULTS); d.update(kw)
        o = _ffi.AprilxVadOptions(C.sizeof(_ffi.AprilxVadOptions) if size is None else size, d["band_lo_hz"], d["band_hi_hz"], d["onset_db"], d["offset_db"],
                                  d["onset_ms"], d["hangover_ms"], d["min_energy"], flags)
        return int(L.aprilx_session_set_vad(a.s._handle, C.byref(o), A._VAD_HANDLER if handler else C.cast(None, _ffi.VAD_HANDLER), id(a.s)))
    out["bad"] = [raw(size=8), raw(flags=2), raw(handler=False), raw(band_hi_hz=sr / 2 + 1.0), raw(band_lo_hz=5.0, band_hi_hz=6.0), raw(offset_db=6.0),
                  raw(onset_ms=5), raw(hangover_ms=20000), raw(min_energy=float("nan"))]
    out["after_bad"] = a.s.vad_info()["onset_frames"]            # nothing changed
    out["set"] = raw(onset_ms=80)
    out["after_set"] = a.s.vad_info()["onset_frames"]
    a.s.feed_pcm16(pcm[:sr])
    out["after_feed"] = raw(onset_ms=50)                          # audio fed since the last completed flush: refused
    out["off_after_feed"] = int(L.aprilx_session_set_vad(a.s._handle, None, C.cast(None, _ffi.VAD_HANDLER), None))
    out["still"] = a.s.vad_info()["onset_frames"]
    a.s.feed_pcm16(pcm[sr:]); a.s.flush()
    out["used"] = list(m.vad_stats())[:2]
    out["frames_seen"] = a.s.frames_seen()
    out["after_flush"] = raw(onset_ms=50)
    out["counters_restart"] = [a.s.vad_info()["segments"], a.s.vad_info()["speech_frames"], a.s.vad_info()["frames_seen"]]
    a.s.set_vad(None)
    out["off"] = a.s.vad_info()
    before = list(m.vad_stats())[:2]
    a.s.feed_pcm16(pcm); a.s.flush()
    out["off_launches_nothing"] = list(m.vad_stats())[:2] == before
    out["frames_seen_runs_on"] = a.s.frames_seen()
    # a profiled pass accounts the kernel's time
    m.profile(1)
    b = Run(m, vad=True)
    b.s.feed_pcm16(pcm); b.s.flush()
    m.profile(0)
    out["profiled_ms"] = m.vad_stats()[2]
    out["events"] = [len(a.vad), len(b.vad)]
    out["mismatch"] = int(m.stats().replay_mismatch)
    return out


def main():
    path, mode = sys.argv[1], sys.argv[2]
    m = A.Model(path)
    if mode == "kernel":
        res = mode_kernel(m)
    elif mode == "live":
        res = {c: mode_live(m, sys.argv[3], c) for c in sys.argv[4:]}
    else:
        res = mode_rules(m)
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
