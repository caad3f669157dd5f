"""Worker for tests/test_gpu_resample.py: sessions with an input rate of their own (aprilx_session_set_input_rate) and the device
resampler (aprilx_resample), one scenario per process.  Prints one line "RESULT <json>".
usage: resample_worker.py model.april mode [rate ...]
modes: kernel | exact RATE... | equiv RATE | edges RATE | extremes | group | long | async | rules

The conversion's expected output comes from the CPU model of the contract (oracle/orc_resample.c), never from the device kernel."""
import hashlib
import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import april_asr_amd as A  # noqa: E402
from conftest import speech_like_pcm  # noqa: E402
from oracle import orc_py as O  # noqa: E402

RATES = [8000, 11025, 22050, 32000, 44100, 48000, 96000]

# bit-exact kernel matrix: model rate -> input rates.  16204 Hz at 16 kHz: L = 4000 > 1 with 2K = 78, not a multiple of 4 (the
# scalar tail behind the float4 loop); 4004 / 383996 Hz: L = 4000 (the largest phase tables); 384000 Hz: K = 854 (the longest
# chains); 328000 Hz at 8 kHz: 16 288 LDS floats, the largest span resample_plan accepts
EXACT_MATRIX = {16000: [4000, 4004, 8000, 11025, 12000, 16204, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 192000, 383996, 384000],
                44100: [8000, 16000, 48000, 384000],
                8000: [16000, 48000, 328000]}
EXACT_CONTENTS = ["noise", "square", "min", "max", "first", "last", "speech"]
LONG_SECONDS = 3.0


def exact_lengths(rate, sr):
    """segment lengths of the bit-exact matrix: 0, 1, K - 1, K, K + 1, 2K, the lengths whose output count is (the nearest count
    reachable to) 255, 256, 257, 511, 512, 513 -- the edges of the kernel's 256-output blocks -- and one long segment"""
    L, M, K = O.resample_lmk(rate, sr)
    ns = [0, 1, K - 1, K, K + 1, 2 * K] + [c * M // L for c in (255, 256, 257, 511, 512, 513)] + [int(LONG_SECONDS * rate)]
    return sorted(set(n for n in ns if n >= 0))


def exact_content(kind, n, seed, rate):
    """int16 segment of n samples at `rate`: full-scale noise (half of it at the rails: the filtered sum clamps on both sides), a full-scale
    square wave, constant -32768 / 32767, a single full-scale impulse at the first / last sample (the zero padding at either
    segment edge), speech-like PCM"""
    rng = np.random.RandomState(seed)
    if kind == "noise":
        # each value held for rate // 4000 samples: the noise keeps its power below 2 kHz, inside every passband, however far the
        # input rate lies above the model's
        hold = max(1, rate // 4000)
        m = -(-n // hold)
        x = rng.randint(-32768, 32768, size=m)
        rails = rng.rand(m) < 0.5
        x[rails] = np.where(rng.rand(int(rails.sum())) < 0.5, -32768, 32767)
        return np.repeat(x, hold)[:n].astype(np.int16)
    if kind == "square":
        period = 2 * (7 + seed % 23)
        return np.where((np.arange(n) // (period // 2)) % 2 == 0, 32767, -32768).astype(np.int16)
    if kind in ("min", "max"):
        return np.full(n, -32768 if kind == "min" else 32767, np.int16)
    if kind in ("first", "last"):
        x = np.zeros(n, np.int16)
        if n:
            x[0 if kind == "first" else n - 1] = -32768 if seed % 2 else 32767
        return x
    return speech_like_pcm(n / float(rate) + 0.01, seed=seed, rate=rate)[:n] * 2 if n else np.zeros(0, np.int16)


def exact_cases(rate, sr):
    """(length, content, samples) of the bit-exact kernel test at one (input rate, model rate) pair: every content at every short
    length, noise and speech on the long segment"""
    long_n = int(LONG_SECONDS * rate)
    for n in exact_lengths(rate, sr):
        for kind in EXACT_CONTENTS:
            if n == long_n and kind not in ("noise", "speech"):
                continue
            yield n, kind, exact_content(kind, n, seed=(rate * 31 + n * 7 + EXACT_CONTENTS.index(kind)) % (2 ** 31), rate=rate)


def oracle_resample(x, rate, sr):
    """the segment converted by the CPU model of the contract with the library's exported table"""
    if rate == sr:
        return np.array(x, np.int16)
    return O.resample(A.resampler_taps(rate, sr)[3], rate, sr, x)


def reference(x, rate, out_rate):
    """numpy float64 direct evaluation of the contract with the exported table: ceil(n L / M) outputs"""
    L, M, K, taps = A.resampler_taps(rate, out_rate)
    t = taps.astype(np.float64)
    n = x.size
    n_out = -((-n * L) // M)
    j = np.arange(n_out, dtype=np.int64)
    k0, p = (j * M) // L, (j * M) % L
    xp = np.concatenate([np.zeros(K, np.float64), x.astype(np.float64), np.zeros(K + 1, np.float64)])
    acc = np.zeros(n_out, np.float64)
    for i in range(2 * K):
        acc += t[p, i] * xp[k0 - K + 1 + i + K]
    return np.clip(np.rint(acc), -32768, 32767).astype(np.int16), (L, M, K)


def avail(n, L, M, K):
    return -((-(n - K) * L) // M) if n > K else 0


class Run:
    """one session's callbacks (type, token text, logprob bits, flags, time) + optional traced logits"""

    def __init__(self, m, rate=None, trace=True, asynchronous=False):
        self.ev = []
        self.cku = 0

        def h(t, toks):
            if int(t) == 3:
                self.cku += 1
            self.ev.append((int(t), [(x[0], struct.pack("<f", float(x[1])), int(x[2]), int(x[3])) for x in toks]))
        self.s = A.Session(m, h, raw_events=True, asynchronous=asynchronous, no_rt=asynchronous, input_sample_rate=rate)
        self.trace = trace
        if trace:
            self.s.trace_logits(40000)

    def play(self, ops):
        for op in ops:
            if op is None:
                self.s.flush()
            else:
                self.s.feed_pcm16(op)
        self.s.drain()
        return self

    def digest(self, frames=True):
        h = hashlib.sha256(repr(self.ev).encode())
        if frames:
            h.update(self.s.frames().tobytes())
        if self.trace:
            h.update(self.s.traced_logits().tobytes())
        return h.hexdigest()


def mode_kernel(m, sr):
    out = {}
    rng = np.random.RandomState(7)
    for rate in RATES:
        x = np.concatenate([speech_like_pcm(1.3, seed=rate, rate=rate), (rng.standard_normal(rate // 3) * 6000).clip(-32768, 32767).astype(np.int16)])
        x = x[: x.size - 1]                                    # (an odd length)
        got = m.resample(x, rate)
        want, (L, M, K) = reference(x, rate, sr)
        d = np.abs(got.astype(np.int64) - want.astype(np.int64)) if got.size == want.size else np.array([99999])
        # full-scale square wave: the float64 sum overshoots past int16 near the edges and is clamped
        period = max(2, rate // 500)
        sq = np.where((np.arange(rate // 2) // (period // 2)) % 2 == 0, 32767, -32768).astype(np.int16)
        gsq = m.resample(sq, rate)
        wsq, _ = reference(sq, rate, sr)
        dsq = np.abs(gsq.astype(np.int64) - wsq.astype(np.int64)) if gsq.size == wsq.size else np.array([99999])
        out[str(rate)] = dict(n=int(x.size), n_out=int(got.size), want=int(-((-x.size * L) // M)), max_diff=int(d.max()),
                              exact=float((d == 0).mean()), sq_n=int(gsq.size), sq_want=int(wsq.size), sq_max_diff=int(dsq.max()),
                              sq_exact=float((dsq == 0).mean()), sq_clamped=int(((wsq == 32767) | (wsq == -32768)).sum()),
                              sq_clamped_equal=bool(((gsq == 32767) == (wsq == 32767)).all() and ((gsq == -32768) == (wsq == -32768)).all()))
    # tones at 48 kHz -> 16 kHz, after int16 rounding
    L, M, K, _ = A.resampler_taps(48000, sr)
    n = 48000 * 2
    t = np.arange(n) / 48000.0
    x = np.rint(10000 * np.sin(2 * np.pi * 1000 * t)).astype(np.int16)
    y = m.resample(x, 48000).astype(np.float64)
    ty = np.arange(y.size) / float(sr)
    ideal = 10000 * np.sin(2 * np.pi * 1000 * ty)
    e = 2 * K
    core = slice(e, y.size - e)
    snr = 10 * np.log10(np.sum(ideal[core] ** 2) / np.sum((y[core] - ideal[core]) ** 2))
    x2 = np.rint(10000 * np.sin(2 * np.pi * 8800 * t)).astype(np.int16)
    y2 = m.resample(x2, 48000).astype(np.float64)
    rms2 = float(np.sqrt(np.mean(y2[core] ** 2)))
    out["tone"] = dict(snr_db=float(snr), stop_rms=rms2)
    return out


def mode_exact(m, sr, rates):
    """the device kernel (aprilx_resample) against the CPU model of the contract, every output bit, over exact_cases; and the
    entry point's edges: n = 0, a cap one below the output count (refused, buffer untouched), a refused rate"""
    out = {}
    for rate in rates:
        L, M, K, taps = A.resampler_taps(rate, sr)
        cases = []
        for n, kind, x in exact_cases(rate, sr):
            want = O.resample(taps, rate, sr, x)
            got = m.resample(x, rate)
            same = got.size == want.size
            diff = int((got != want).sum()) if same else -1
            clamp = (int((want == -32768).sum()), int((want == 32767).sum()))
            cases.append([n, kind, int(want.size), int(got.size), diff, clamp[0], clamp[1]])
        # aprilx_resample's edges
        Lb = m._L
        x = exact_content("noise", 4 * K + 3, seed=rate, rate=rate)
        n_out = -((-x.size * L) // M)
        buf = np.full(n_out + 8, 12345, np.int16)
        e = dict(zero=int(Lb.aprilx_resample(m._handle, rate, x.ctypes.data, 0, buf.ctypes.data, buf.size)),
                 short_cap=int(Lb.aprilx_resample(m._handle, rate, x.ctypes.data, x.size, buf.ctypes.data, n_out - 1)),
                 untouched=bool((buf == 12345).all()),
                 exact_cap=int(Lb.aprilx_resample(m._handle, rate, x.ctypes.data, x.size, buf.ctypes.data, n_out)),
                 n_out=int(n_out))
        e["exact_cap_equal"] = bool((buf[:n_out] == O.resample(taps, rate, sr, x)).all() and (buf[n_out:] == 12345).all())
        out[str(rate)] = dict(lmk=[L, M, K], cases=cases, edges=e)
    refused = 383996 if sr == 44100 else (336000 if sr == 8000 else 4001)
    x = exact_content("noise", 1000, seed=1, rate=sr)
    buf = np.zeros(1000, np.int16)
    out["refused"] = [refused, int(m._L.aprilx_resample(m._handle, refused, x.ctypes.data, x.size, buf.ctypes.data, buf.size))]
    return out


def equiv_ops(m, rate, sr, segments=None):
    """A: the session at `rate`, random feed sizes (1-sample feeds included), flush, a second segment, flush.  B: the default session
    fed after each of A's feeds exactly the model-rate samples that became available there (the CPU model's conversion of the whole
    segment cut by the availability rule), with the same flush points."""
    L, M, K, _ = A.resampler_taps(rate, sr)
    rng = np.random.RandomState(rate % (2 ** 31))
    sizes = [1, 1, 2, 7, 160, rate // 50, rate // 10, rate // 10, rate // 4, rate // 2]
    ops_a, ops_b = [], []
    if segments is None:
        segments = (speech_like_pcm(2.6, seed=1, rate=rate), speech_like_pcm(1.7, seed=2, rate=rate))
    for seg in segments:
        y = oracle_resample(seg, rate, sr)
        pos = given = 0
        while pos < seg.size:
            piece = seg[pos: pos + int(rng.choice(sizes))]
            pos += piece.size
            ops_a.append(piece)
            av = avail(pos, L, M, K)
            ops_b.append(y[given:av])
            given = av
        ops_a.append(None)
        if seg.size:                # (an empty feed still opens a segment, as in the reference: B feeds only where A did)
            ops_b.append(y[given:])
        ops_b.append(None)
    return ops_a, ops_b


def mode_equiv(m, sr, rate, segments=None):
    ops_a, ops_b = equiv_ops(m, rate, sr, segments)
    a = Run(m, rate).play(ops_a)
    b = Run(m).play(ops_b)
    fa, fb = a.s.frames(), b.s.frames()
    la, lb = a.s.traced_logits(), b.s.traced_logits()
    return dict(events_equal=a.ev == b.ev, n_events=len(a.ev), n_tokens=sum(len(t) for _, t in a.ev),
                frames_equal=bool(fa.shape == fb.shape and (fa.view(np.uint32) == fb.view(np.uint32)).all()), n_frames=int(fa.shape[0]),
                logits_equal=bool(la.shape == lb.shape and (la.view(np.uint32) == lb.view(np.uint32)).all()), n_logits=int(la.shape[0]),
                n_frames_default=int(fb.shape[0]), n_logits_default=int(lb.shape[0]),
                feeds=len(ops_a), rate=a.s.input_rate)


def mode_edges(m, sr, rate):
    """segments that stress FrameBook's framing and compaction: one shorter than K (5 samples), an empty one (two flushes in a row),
    one of a single sample, and segments whose flush falls inside a filterbank window (lengths that are no multiple of the frame
    shift at either rate), so that one window is filled from two descriptors and the zeros behind the first segment"""
    def seg(seconds, seed):
        return speech_like_pcm(seconds, seed=seed, rate=rate)
    segments = [seg(0.01, 21)[:5], np.zeros(0, np.int16), seg(0.01, 22)[:1], seg(0.6, 23)[: int(0.6 * rate) - 3],
                seg(0.01, 24)[:5], seg(1.3, 25)[: int(1.3 * rate) + 7], np.zeros(0, np.int16), seg(0.4, 26)[: int(0.4 * rate) - 1]]
    return mode_equiv(m, sr, rate, segments)


EXTREME_RATES = [4000, 4004, 384000, 383996, None, 48000]


def mode_extremes(m, sr):
    """one pipelined group whose sessions are at the extreme rates (the largest phase tables, the longest chains, upsampling with a
    small L, a default session) mixed in one launch -- lds_floats is the maximum over descriptors of different (L, M, K) while every
    block sizes its own span: each session gives the callbacks, feature rows and logits of the default session fed the CPU model's
    conversion as it becomes available"""
    n, steps = 2 * len(EXTREME_RATES), 12
    rates = [EXTREME_RATES[i % len(EXTREME_RATES)] for i in range(n)]
    pcm = [speech_like_pcm(1.2, seed=300 + i, rate=r or sr) for i, r in enumerate(rates)]
    step = [(r or sr) // 10 for r in rates]
    runs = [Run(m, r) for r in rates]
    grp = A.SessionGroup([r.s for r in runs])
    for k in range(steps):
        grp.feed_pipelined([pcm[i][k * step[i]:(k + 1) * step[i]] for i in range(n)], 2)
    grp.drain()
    grp.flush()
    grp.drain()
    equal = []
    for i, r in enumerate(rates):
        rate = r or sr
        seg = pcm[i][: steps * step[i]]
        y = oracle_resample(seg, rate, sr)
        L, M, K = O.resample_lmk(rate, sr)
        ops, given = [], 0
        for k in range(steps):
            av = avail((k + 1) * step[i], L, M, K) if r not in (None, sr) else (k + 1) * step[i]
            ops.append(y[given:av])
            given = av
        ops += [y[given:], None]
        b = Run(m).play(ops)
        equal.append(runs[i].digest() == b.digest())
    return dict(rates=[r or 0 for r in rates], equal=equal, n_events=[len(r.ev) for r in runs],
                n_frames=[int(r.s.frames().shape[0]) for r in runs])


GROUP_RATES = [None, 16000, 8000, 22050, 44100, 48000, 11025, 32000]


def group_pcm(i, rate, sr):
    return speech_like_pcm(2.0, seed=100 + i, rate=rate or sr)


def mode_group(m, sr):
    n, steps = 32, 20
    rates = [GROUP_RATES[i % len(GROUP_RATES)] for i in range(n)]
    pcm = [group_pcm(i, r, sr) for i, r in enumerate(rates)]
    step = [(r or sr) // 10 for r in rates]

    def group_run(idx):
        runs = [Run(m, rates[i], trace=False) for i in idx]
        grp = A.SessionGroup([r.s for r in runs])
        for k in range(steps):
            grp.feed_pipelined([pcm[i][k * step[i]:(k + 1) * step[i]] for i in idx], 2)
        grp.drain()
        grp.flush()
        grp.drain()
        return [r.digest(frames=False) for r in runs]

    mixed = group_run(list(range(n)))
    single = []
    for i in range(n):
        ops = [pcm[i][k * step[i]:(k + 1) * step[i]] for k in range(steps)] + [None]
        single.append(Run(m, rates[i], trace=False).play(ops).digest(frames=False))
    defaults = [i for i in range(n) if rates[i] in (None, sr)]
    plain = group_run(defaults)
    return dict(rates=[r or 0 for r in rates], mixed_equals_single=[mixed[i] == single[i] for i in range(n)],
                defaults_equal_plain=[mixed[i] == plain[k] for k, i in enumerate(defaults)],
                distinct=len(set(mixed)))


def long_ops(seconds=60):
    x = speech_like_pcm(seconds, seed=9, rate=48000)
    return x


def mode_long(m, sr):
    x = long_ops()
    one = Run(m, 48000, trace=False).play([x, None])
    st = m.stats()
    res = dict(one=one.digest(frames=False), n_events=len(one.ev), lm_chunks=int(st.lm_chunks))
    if os.environ.get("APRIL_STAGE_LIMIT_SAMPLES"):
        return res
    pieces = [x[i:i + 4800] for i in range(0, x.size, 4800)] + [None]
    res["pieces"] = Run(m, 48000, trace=False).play(pieces).digest(frames=False)
    return res


def mode_async(m, sr):
    # 2.8 s in all: below the 3 s the asynchronous session may hold, so however far its feeds run ahead of the stepping thread, none
    # is refused (a refused feed is dropped, as in the reference, and the two runs would then differ for that reason alone)
    x = speech_like_pcm(2.8, seed=5, rate=44100)
    ops = [x[i:i + 4410] for i in range(0, x.size, 4410)] + [None]
    sync = Run(m, 44100, trace=False).play(ops)
    asy = Run(m, 44100, trace=False, asynchronous=True).play(ops)
    # CANT_KEEP_UP: an asynchronous session refuses a push that would make it hold 3 s of audio at ITS rate (132 300 at 44.1 kHz)
    ck = {}
    for cnt in (48000, 132299, 132300):
        r = Run(m, 44100, trace=False, asynchronous=True)
        r.s.feed_pcm16(speech_like_pcm(cnt / 44100.0 + 0.01, seed=3, rate=44100)[:cnt])
        r.s.drain()
        ck[str(cnt)] = r.cku
        r.s.close()
    r = Run(m, None, trace=False, asynchronous=True)
    r.s.feed_pcm16(speech_like_pcm(3.01, seed=3)[:48000])
    r.s.drain()
    ck["default_48000"] = r.cku
    return dict(async_equals_sync=asy.ev == sync.ev, n_events=len(sync.ev), async_refused=asy.cku, cant_keep_up=ck)


def mode_rules(m, sr):
    res = {}
    ev = []
    s = A.Session(m, lambda t, k: ev.append(t), raw_events=True)
    L = s._L
    res["fresh"] = L.aprilx_session_set_input_rate(s._handle, 48000)
    res["rate_after_set"] = s.input_rate
    s.feed_pcm16(speech_like_pcm(0.3, rate=48000))
    res["after_feed"] = L.aprilx_session_set_input_rate(s._handle, 44100)
    res["rate_after_refusal"] = s.input_rate
    s.flush()
    res["after_flush"] = L.aprilx_session_set_input_rate(s._handle, 44100)
    res["bad_rates"] = [L.aprilx_session_set_input_rate(s._handle, r) for r in (0, 3999, 384001, 4001)]
    res["back_to_model_rate"] = L.aprilx_session_set_input_rate(s._handle, sr)
    res["rate_default"] = s.input_rate
    s.close()
    # a session set to the model rate is identical to one never set (including after a detour through 48 kHz)
    x = speech_like_pcm(3.0, seed=11)
    ops = [x[i:i + 1600] for i in range(0, x.size, 1600)] + [None]
    never = Run(m).play(ops).digest()
    set_sr = Run(m, sr).play(ops).digest()
    x48 = speech_like_pcm(1.0, seed=12, rate=48000)
    d = Run(m, 48000).play([x48, None])
    d.s.set_input_rate(sr)
    d2 = Run(m).play([m.resample(x48, 48000), None])
    res["set_model_rate_equal"] = never == set_sr
    # a detour through 48 kHz and back: the same callbacks, frames and logits as the default session fed the converted audio
    d.play(ops)
    d2.play(ops)
    res["detour_equal"] = d.digest() == d2.digest()
    # the profiled path times the resample launches in their own class
    m.profile(1)
    Run(m, 44100, trace=False).play([speech_like_pcm(1.0, seed=13, rate=44100), None])
    m.profile(0)
    st = m.stats()
    res["resample_launches"] = int(st.resample_launches)
    res["resample_ms"] = float(st.resample_ms)
    return res


def main():
    path, mode = sys.argv[1], sys.argv[2]
    m = A.Model(path)
    sr = int(m.dims.sample_rate)
    if mode == "kernel":
        res = mode_kernel(m, sr)
    elif mode == "exact":
        res = mode_exact(m, sr, [int(r) for r in sys.argv[3:]])
    elif mode == "equiv":
        res = mode_equiv(m, sr, int(sys.argv[3]))
    elif mode == "edges":
        res = mode_edges(m, sr, int(sys.argv[3]))
    elif mode == "extremes":
        res = mode_extremes(m, sr)
    else:
        res = dict(group=mode_group, long=mode_long, asynchronous=mode_async, rules=mode_rules)[mode](m, sr)
    print("RESULT " + json.dumps(res), flush=True)
    # close every session, then the model, while all of them are alive: left to the interpreter's last collection, the sessions
    # (in reference cycles through their handlers) and the model would be finalized in no particular order
    m.close()


if __name__ == "__main__":
    main()
