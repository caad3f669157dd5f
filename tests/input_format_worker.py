"""Worker for tests/test_gpu_input_format.py: sessions with an input format (aprilx_session_set_input_format) and the device decode
(aprilx_decode), one scenario per process.  Prints one line "RESULT <json>".
usage: input_format_worker.py model.april mode [args ...]

What a format must decode to comes from the numpy statement of the contract (tests/input_format_ref.py), never from the product."""
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
from oracle import orc_py as O  # noqa: E402
from conftest import speech_like_pcm  # noqa: E402
import input_format_ref as R  # noqa: E402

# every (encoding, channels, channel): channels 1, 2, 3, 8 x the downmix, the first and the last channel
COMBOS = [(e, c, ch) for e in R.ENCODINGS for c in (1, 2, 3, 8) for ch in sorted({-1, 0, c - 1})]
KERNEL_FRAMES = [0, 1, 63, 64, 65, 255, 256, 257, 4097]          # the edges of the kernel's 256-frame tile and of a wave


def raw_values(enc, n, rng):
    """n values of `enc` that reach every branch of its rule"""
    if enc == "s16":
        x = rng.randint(-32768, 32768, size=n)
        x[rng.rand(n) < 0.1] = -32768
        x[rng.rand(n) < 0.1] = 32767
        return x.astype("<i2")
    if enc == "f32":
        x = rng.uniform(-1.1, 1.1, size=n).astype(np.float32)
        k = rng.rand(n)
        ties = ((rng.randint(-32770, 32770, size=n) + 0.5) / 32768.0).astype(np.float32)
        bits = rng.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32)
        x = np.where(k < 0.25, ties, x)
        x = np.where(k > 0.85, bits, x)
        edge = np.array([v for v, _ in R.F32_VALUES] + [p / 32768.0 for p, _ in R.F32_PRODUCTS], np.float32)
        m = min(n, edge.size)
        x[:m] = edge[:m]
        return x.astype("<f4")
    x = rng.randint(0, 256, size=n)
    m = min(n, 256)
    x[:m] = rng.permutation(256)[:m]
    return x.astype(np.uint8)


def mode_kernel(m):
    bad, calls = [], 0
    for ci, (enc, c, ch) in enumerate(COMBOS):
        for frames in KERNEL_FRAMES:
            raw = raw_values(enc, frames * c, np.random.RandomState(1000 * ci + frames))
            got = m.decode(raw, (enc, c, ch))
            want = R.decode(raw, enc, c, ch)
            calls += 1
            if got.shape != want.shape or not (got == want).all():
                bad.append([enc, c, ch, frames, int((got != want).sum()) if got.shape == want.shape else -1])
    # all 256 codes and the literal values through the kernel
    lit = []
    for enc in ("mulaw", "alaw"):
        codes = np.arange(256, dtype=np.uint8)
        lit.append(bool((m.decode(codes, (enc, 1, 0)) == R.decode(codes, enc)).all()))
    lit.append([int(m.decode(bytes([code]), (enc, 1, 0))[0]) for enc, code, _ in R.LITERALS] == [w for _, _, w in R.LITERALS])
    lit.append([int(m.decode(np.array([p / 32768.0], np.float32), ("f32", 1, 0))[0]) for p, _ in R.F32_PRODUCTS] == [w for _, w in R.F32_PRODUCTS])
    lit.append([int(m.decode(np.array([x], np.float32), ("f32", 1, 0))[0]) for x, _ in R.F32_VALUES] == [w for _, w in R.F32_VALUES])
    # refusals of aprilx_decode
    L = m._L
    out = np.zeros(8, np.int16)
    data = np.zeros(64, np.uint8)

    def call(e, c, ch, nbytes, cap):
        f = _ffi.AprilxInputFormat(C.sizeof(_ffi.AprilxInputFormat), e, c, ch)
        return int(L.aprilx_decode(m._handle, C.byref(f), data.ctypes.data, nbytes, out.ctypes.data, cap))
    refusals = [call(3, 3, 0, 16, 8), call(1, 1, 0, 9, 8), call(4, 1, 0, 4, 8), call(0, 2, 2, 4, 8), call(0, 1, 0, 0, 0), call(0, 1, 0, 8, 8)]
    return dict(bad=bad, calls=calls, literals=lit, refusals=refusals)


class Run:
    """one session's callbacks (type, token text, logprob bits, flags, time)"""

    def __init__(self, m, fmt=None, rate=None, asynchronous=False):
        self.ev = []
        self.cku = 0

        def h(t, toks):
            if int(t) == 3:
                self.cku += 1
            self.ev.append((int(t), [(x[0], struct.pack("<f", float(x[1])), int(x[2]), int(x[3])) for x in toks]))
        kw = dict(input_format=fmt[0], channels=fmt[1], channel=fmt[2]) if fmt else {}
        self.s = A.Session(m, h, raw_events=True, asynchronous=asynchronous, no_rt=asynchronous, input_sample_rate=rate, **kw)


def same(a, b):
    fa, fb = a.s.frames(), b.s.frames()
    return dict(events=a.ev == b.ev, frames=bool(fa.shape == fb.shape and (fa.view(np.uint32) == fb.view(np.uint32)).all()),
                chunks=a.s.chunks() == b.s.chunks())


def cuts(n, chunking, unit, seed):
    """frame boundaries of the feeds of n frames: 100 ms feeds, irregular feeds (single-frame feeds included), or one feed"""
    if chunking == "whole":
        return [0, n]
    if chunking == "100ms":
        return list(range(0, n, unit)) + [n]
    rng = np.random.RandomState(seed)
    sizes = [1, 1, 2, 7, 159, unit // 2, unit, unit, 3 * unit, 5 * unit + 3]
    at, out = 0, [0]
    while at < n:
        at = min(n, at + int(rng.choice(sizes)))
        out.append(at)
    return out


def mode_live(m, mode, chunking):
    """one pair of sessions per combination: A has the format and is fed the raw bytes, B has none and is fed the
    int16 the numpy statement decodes from the same bytes.  Two segments with a flush between them and one at the end."""
    sr = int(m.dims.sample_rate)
    asynchronous = mode == "async"
    segs = [(0, int(1.2 * sr)), (int(1.2 * sr), 2 * sr)]
    pairs, raws, decs = [], [], []
    for i, (enc, c, ch) in enumerate(COMBOS):
        pcm = O.lcg_pcm16_fast(2 * sr, seed=100 + i)
        raw = R.make_raw(pcm, enc, c, seed=i)
        raws.append(raw); decs.append(R.decode(raw, enc, c, ch))
        pairs.append((Run(m, (enc, c, ch), asynchronous=asynchronous), Run(m, None, asynchronous=asynchronous)))
    fbytes = [c * R.BYTES[enc] for enc, c, _ in COMBOS]
    sessions = [r.s for p in pairs for r in p]
    grp = A.SessionGroup(sessions)
    # the A sessions are fed in one group call in bytes, the B sessions through the PCM16 entry points that were there before
    grp_a, grp_b = A.SessionGroup([a.s for a, _ in pairs]), A.SessionGroup([b.s for _, b in pairs])
    fed = 0
    for si, (s0, s1) in enumerate(segs):
        bounds = cuts(s1 - s0, chunking, sr // 10, seed=si)
        for f0, f1 in zip(bounds[:-1], bounds[1:]):
            bufs = []
            for i in range(len(COMBOS)):
                bufs.append(raws[i][(s0 + f0) * fbytes[i]:(s0 + f1) * fbytes[i]])
                bufs.append(decs[i][s0 + f0:s0 + f1])
            fed += (f1 - f0) * len(COMBOS)
            if mode == "sync":
                grp_a.feed_bytes(bufs[0::2]); grp_b.feed(bufs[1::2])
            elif mode == "pipe2":
                grp_a.feed_bytes(bufs[0::2], 2); grp_b.feed_pipelined(bufs[1::2], 2)
            else:
                for k, (a, b) in enumerate(pairs):
                    a.s.feed(bufs[2 * k]); b.s.feed_pcm16(bufs[2 * k + 1])
        grp.drain()
        grp.flush()
        grp.drain()
    eq = [same(a, b) for a, b in pairs]
    launches, frames, _ = m.decode_stats()
    # ({S16, 1, 0} reads back as no format: that pair is two plain sessions, and its frames are not decoded)
    formatted = sum(1 for a, _ in pairs if a.s.input_format() is not None)
    res = dict(equal=eq, tokens=[sum(len(t) for _, t in b.ev) for _, b in pairs], chunks=[b.s.chunks() for _, b in pairs],
               cku=sum(a.cku + b.cku for a, b in pairs), mismatch=int(m.stats().replay_mismatch), launches=launches, frames=frames,
               fed=fed // len(COMBOS) * formatted, formats=[a.s.input_format() for a, _ in pairs])
    for r in sessions:
        r.close()
    return res


def mode_rates(m):
    """a format together with an input rate: the raw frames are the resampler's input"""
    res = {}
    for name, fmt, rate in (("mulaw8k", ("mulaw", 2, 1), 8000), ("f32_44k1", ("f32", 2, -1), 44100)):
        pcm = speech_like_pcm(2.0, seed=41, rate=rate) * 2
        raw = R.make_raw(pcm, fmt[0], fmt[1], seed=5)
        dec = R.decode(raw, *fmt)
        fb = fmt[1] * R.BYTES[fmt[0]]
        a, b = Run(m, fmt, rate=rate), Run(m, None, rate=rate)
        bounds = cuts(dec.size, "irregular", rate // 10, seed=2)
        half = len(bounds) // 2
        for k, (f0, f1) in enumerate(zip(bounds[:-1], bounds[1:])):
            a.s.feed(raw[f0 * fb:f1 * fb]); b.s.feed_pcm16(dec[f0:f1])
            if k == half:
                a.s.flush(); b.s.flush()
        a.s.flush(); b.s.flush()
        res[name] = dict(same(a, b), tokens=sum(len(t) for _, t in b.ev), chunks=b.s.chunks(), rate=a.s.input_rate, fmt=a.s.input_format())
        # the other order: rate after format
        c = A.Session(m, lambda t, k: None, raw_events=True, input_format=fmt[0], channels=fmt[1], channel=fmt[2])
        c.set_input_rate(rate)
        res[name]["other_order"] = [c.input_rate, c.input_format()]
        c.close(); a.s.close(); b.s.close()
    res["mismatch"] = int(m.stats().replay_mismatch)
    return res


def mode_rules(m):
    sr = int(m.dims.sample_rate)
    L = m._L
    res = {}

    def setf(s, enc, c, ch, size=None):
        f = _ffi.AprilxInputFormat(C.sizeof(_ffi.AprilxInputFormat) if size is None else size, enc, c, ch)
        return int(L.aprilx_session_set_input_format(s._handle, C.byref(f)))

    a = Run(m)
    s = a.s
    res["fresh_none"] = s.input_format()
    res["set"] = setf(s, 1, 2, 1)
    res["read"] = s.input_format()
    # every bad value is refused and the format stays
    res["bad"] = [setf(s, 4, 1, 0), setf(s, 0, 0, 0), setf(s, 0, 9, 0), setf(s, 0, 2, 2), setf(s, 0, 2, -2), setf(s, 1, 1, 0, size=12)]
    res["after_bad"] = s.input_format()
    pcm = O.lcg_pcm16_fast(2 * sr, seed=77)
    raw = R.make_raw(pcm, "mulaw", 2, seed=9)
    dec = R.decode(raw, "mulaw", 2, 1)
    b = Run(m)
    # a partial frame is refused and nothing is queued; the whole feed afterwards is as if it never happened
    res["partial"] = int(L.aprilx_session_feed_bytes(s._handle, raw.ctypes.data, 3201))
    res["settable_after_partial"] = setf(s, 1, 2, 1)
    half = sr
    s.feed(raw[:2 * half]); b.s.feed_pcm16(dec[:half])
    res["after_feed"] = setf(s, 2, 1, 0)
    res["after_refusal"] = s.input_format()
    # aas_feed_pcm16 on a session with a format: 2 x short_count bytes at the pointer (an even byte count of mu-law, 2 channels)
    rest = np.ascontiguousarray(raw[2 * half:])
    L.aas_feed_pcm16(s._handle, rest.ctypes.data, rest.size // 2); b.s.feed_pcm16(dec[half:])
    s.flush(); b.s.flush()
    res["equal"] = same(a, b)
    res["tokens"] = sum(len(t) for _, t in b.ev)
    res["chunks"] = b.s.chunks()
    res["after_flush"] = setf(s, 2, 1, 0)
    res["read_after_flush"] = s.input_format()
    res["default_struct"] = setf(s, 0, 1, 0)
    res["default_reads"] = s.input_format()
    res["null"] = int(L.aprilx_session_set_input_format(s._handle, None))
    # the legacy entry point with a partial frame: logged and dropped, the session goes on
    t = Run(m, ("alaw", 3, 0))
    x = np.zeros(8, np.uint8)
    L.aas_feed_pcm16(t.s._handle, x.ctypes.data, 4)           # 8 bytes: not a whole number of 3-byte frames
    res["dropped_still_settable"] = setf(t.s, 2, 3, 1)
    # the group feed in bytes: one partial frame refuses the whole call
    g = A.SessionGroup([t.s, b.s])
    try:
        g.feed_bytes([np.zeros(6, np.uint8), np.zeros(3, np.uint8)])
        res["group_partial"] = 0
    except ValueError:
        res["group_partial"] = -1
    res["group_nothing_queued"] = setf(t.s, 2, 3, 1)
    out = _ffi.AprilxInputFormat()
    res["getter_bad_args"] = [int(L.aprilx_session_input_format(None, C.byref(out))), int(L.aprilx_session_input_format(s._handle, None))]
    res["mismatch"] = int(m.stats().replay_mismatch)
    for r in (a, b, t):
        r.s.close()
    return res


def mode_plain(m):
    """plain sessions issue no decode work; with profiling on, a formatted session's launches are timed in their own class"""
    sr = int(m.dims.sample_rate)
    pcm = O.lcg_pcm16_fast(2 * sr, seed=3)
    a = Run(m)
    for i in range(0, pcm.size, sr // 10):
        a.s.feed_pcm16(pcm[i:i + sr // 10])
    a.s.flush()
    c = Run(m, ("s16", 1, 0))                                    # the default, set explicitly: still no decode work
    c.s.feed(pcm); c.s.flush()
    res = dict(plain=list(m.decode_stats()), chunks=a.s.chunks(), default_equal=a.ev == c.ev)
    m.profile(1)
    b = Run(m, ("mulaw", 1, 0))
    b.s.feed(R.encode(pcm, "mulaw")); b.s.flush()
    m.profile(0)
    res["profiled"] = list(m.decode_stats())
    for r in (a, b, c):
        r.s.close()
    return res


def mode_limit(m):
    """one feed of more than the staging limit (APRIL_STAGE_LIMIT_SAMPLES, set by the test) into an F32 session with 8 channels, the
    format with the most bytes per frame, against its PCM16 twin"""
    sr = int(m.dims.sample_rate)
    fmt = ("f32", 8, -1)
    pcm = O.lcg_pcm16_fast(2 * sr, seed=8)
    raw = R.make_raw(pcm, fmt[0], fmt[1], seed=4)
    dec = R.decode(raw, *fmt)
    a, b = Run(m, fmt), Run(m)
    a.s.feed(raw); b.s.feed_pcm16(dec)
    a.s.flush(); b.s.flush()
    res = dict(same(a, b), tokens=sum(len(t) for _, t in b.ev), chunks=b.s.chunks(), bytes=int(raw.size), mismatch=int(m.stats().replay_mismatch),
               limit=os.environ.get("APRIL_STAGE_LIMIT_SAMPLES"), launches=m.decode_stats()[0])
    a.s.close(); b.s.close()
    return res


def main():
    path, mode = sys.argv[1], sys.argv[2]
    m = A.Model(path)
    if mode == "live":
        res = {c: mode_live(m, sys.argv[3], c) for c in sys.argv[4:]}
    else:
        res = dict(kernel=mode_kernel, rates=mode_rates, rules=mode_rules, plain=mode_plain, limit=mode_limit)[mode](m)
    print("RESULT " + json.dumps(res), flush=True)
    m.close()


if __name__ == "__main__":
    main()
