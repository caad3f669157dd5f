"""The tone contract stated in numpy: options -> plan, tables, steps 1-7 per frame, and the event machine.
Written from the text of the contract, not from csrc/tone.h; the CPU and GPU tests hold the product against it on every bit.
All fp32 arithmetic is spelled with np.float32 operands, one operation per statement, so nothing is contracted or widened."""
import numpy as np

F32 = np.float32
ON, OFF = 1, 2
DEFAULTS = dict(min_level_dbfs=-40.0, second_db=10.0, min_share=0.7, tol_hz=20, min_tone_ms=60, min_pause_ms=30)
NAMES = (("dial", 350, 440), ("busy", 480, 620), ("cp425", 425, 0), ("cng", 1100, 0), ("ced", 2100, 0), ("sit1", 950, 0), ("sit2", 1400, 0),
         ("sit3", 1800, 0))


def options(**kw):
    d = dict(DEFAULTS)
    d.update(kw)
    return d


def grid(rate, fft_size):
    """(W, k_lo, F), or None for a refused model"""
    rate, fft_size = int(rate), int(fft_size)
    w = 64 * (fft_size // 64)
    if rate < 6000 or w <= 0 or w * 1000 < 20 * rate or w > 4096:
        return None
    k_lo = -((-300 * w) // rate)
    k_hi = min(2300 * w // rate, w // 2 - 1)
    f = k_hi - k_lo + 1
    if f < 8 or f > 128:
        return None
    return w, k_lo, f


def options_valid(o):
    f = [o["min_level_dbfs"], o["second_db"], o["min_share"]]
    if not all(np.isfinite(F32(v)) for v in f):
        return False
    return bool(-70 <= F32(o["min_level_dbfs"]) <= 0 and 3 <= F32(o["second_db"]) <= 30 and 0 < F32(o["min_share"]) <= 1
                and 1 <= o["tol_hz"] <= 200 and 10 <= o["min_tone_ms"] <= 5000 and 10 <= o["min_pause_ms"] <= 5000)


def make_plan(rate, fft_size, shift_ms, o):
    g = grid(rate, fft_size)
    if g is None or shift_ms <= 0 or not options_valid(o):
        return None
    w, k_lo, f = g
    db = lambda v: float(F32(v))                      # the option as the fp32 the C struct holds
    amp = 32768.0 * 10.0 ** (db(o["min_level_dbfs"]) / 20.0) * w / 2.0
    return dict(W=w, k_lo=k_lo, F=f, half_w=F32(0.5) * F32(w), min_power=F32(amp * amp), second_ratio=F32(10.0 ** (db(o["second_db"]) / 10.0)),
                min_share=F32(o["min_share"]), bin_hz=F32(rate) / F32(w), tol_hz=int(o["tol_hz"]),
                on_frames=max(1, int(o["min_tone_ms"]) // shift_ms), off_frames=max(1, int(o["min_pause_ms"]) // shift_ms))


def tables_f64(w, k_lo, f):
    """[2F][W] in double: row k cos, row F + k sin of 2 pi m / W, m = ((k_lo + k) j) mod W"""
    j = np.arange(w, dtype=np.int64)
    m = ((k_lo + np.arange(f, dtype=np.int64))[:, None] * j[None, :]) % w
    a = 2.0 * np.pi * m.astype(np.float64) / float(w)
    return np.concatenate([np.cos(a), np.sin(a)])


def powers(plan, tables, frames):
    """steps 1 and 2: frames [n][>= W] int16, tables [2F][W] float32 -> [n][F + 1] float32: P[0..F), E"""
    w, f = plan["W"], plan["F"]
    x = np.asarray(frames)[:, :w]
    t = np.asarray(tables, np.float32)
    assert t.shape == (2 * f, w) and x.dtype == np.int16
    out = np.zeros((len(x), f + 1), np.float32)
    idx = np.arange(64)
    for lo in range(0, len(x), 64):                   # (blocks of frames: [64][2F][W] products at a time)
        xf = x[lo:lo + 64].astype(np.float32)
        a = np.zeros((len(xf), 2 * f, 64), np.float32)
        for k in range(0, w, 64):
            m = xf[:, None, k:k + 64] * t[None, :, k:k + 64]
            a = a + m
        for d in (32, 16, 8, 4, 2, 1):
            a = a + a[:, :, idx ^ d]
        c = a[:, :, 0]
        re, im = c[:, :f], c[:, f:]
        rr = re * re
        ii = im * im
        assert a.dtype == np.float32 and rr.dtype == np.float32
        out[lo:lo + 64, :f] = rr + ii
    e = (x.astype(np.int64) ** 2).sum(axis=1)
    out[:, f] = e.astype(np.float32)
    return out


def _hz(plan, P, c):
    f = plan["F"]
    l = P[c - 1] if c > 0 else F32(0)
    r = P[c + 1] if c + 1 < f else F32(0)
    with np.errstate(all="ignore"):
        if r >= l:
            s = np.sqrt(F32(r / P[c]))
            d = F32(s / F32(F32(1) + s))
        else:
            s = np.sqrt(F32(l / P[c]))
            d = -F32(s / F32(F32(1) + s))
        v = F32(F32(F32(F32(plan["k_lo"] + c) + d) * plan["bin_hz"]) + F32(0.5))
    return int(v) if v >= 1 and v < 65536 else 0      # (no number inside 1 .. 65535: no frequency)


def decide(plan, q):
    """steps 3-7 on one row of P[0..F), E: the record (f1, f2)"""
    f = plan["F"]
    P = [F32(v) for v in q[:f]]
    E = F32(q[f])
    with np.errstate(all="ignore"):
        p = 0
        for i in range(1, f):
            if P[i] > P[p]:
                p = i
        if not P[p] >= plan["min_power"]:
            return 0, 0
        qq = -1
        for i in range(f):
            if abs(i - p) >= 3 and (qq < 0 or P[i] > P[qq]):
                qq = i
        dual = not F32(P[qq] * plan["second_ratio"]) < P[p]
        comps = sorted([p, qq]) if dual else [p]
        S = F32(0)
        for c in comps:
            for i in (c - 1, c, c + 1):
                if 0 <= i < f:
                    S = F32(S + P[i])
        if S < F32(plan["min_share"] * F32(E * plan["half_w"])):
            return 0, 0
    hz = [_hz(plan, P, c) for c in comps]
    if 0 in hz:
        return 0, 0
    hz.sort()
    return (hz[0], hz[1]) if dual else (hz[0], 0)


def run(plan, tables, frames):
    """(records [n][2] uint16, powers [n][F + 1])"""
    q = powers(plan, tables, frames)
    return np.array([decide(plan, row) for row in q], np.uint16).reshape(-1, 2), q


def match(a, b, tol):
    return (a[1] == 0) == (b[1] == 0) and abs(a[0] - b[0]) <= tol and abs(a[1] - b[1]) <= tol


def machine():
    return dict(held=None, cand=None, run=0)


def events(plan, shift_ms, t0, records, m):
    """the event machine over the records of frames t0 .. ; m is updated in place.  [(kind, f1, f2, time_ms)]"""
    on, off, tol = plan["on_frames"], plan["off_frames"], plan["tol_hz"]
    out = []
    for i, rec in enumerate(records):
        r = (int(rec[0]), int(rec[1]))
        tonal = r[0] != 0
        t = t0 + i
        if m["held"] is not None:
            m["run"] = 0 if tonal and match(r, m["held"], tol) else m["run"] + 1
            if m["run"] < off:
                continue
            out.append((OFF, m["held"][0], m["held"][1], (t - off + 1) * shift_ms))
            m.update(held=None, cand=None, run=0)     # ... and this frame starts the next candidate run
        if not tonal:
            m.update(cand=None, run=0)
            continue
        if m["cand"] is not None and match(r, m["cand"], tol):
            m["run"] += 1
        else:
            m.update(cand=r, run=1)
        if m["run"] >= on:
            out.append((ON, r[0], r[1], (t - on + 1) * shift_ms))
            m.update(held=r, cand=None, run=0)
    return out


def flush(shift_ms, frames_seen, m):
    out = [(OFF, m["held"][0], m["held"][1], frames_seen * shift_ms)] if m["held"] is not None else []
    m.update(held=None, cand=None, run=0)
    return out


def name(f1, f2, tol=20):
    for n, a, b in NAMES:
        if match((f1, f2), (a, b), tol):
            return n
    return None


def frames_of(pcm, fft_size, shift):
    """frame t = pcm[t shift : t shift + fft_size], every whole frame, as a contiguous [n][fft_size] int16 array"""
    pcm = np.asarray(pcm, np.int16)
    n = (len(pcm) - fft_size) // shift + 1 if len(pcm) >= fft_size else 0
    if n <= 0:
        return np.zeros((0, fft_size), np.int16)
    return np.ascontiguousarray(np.lib.stride_tricks.as_strided(pcm, (n, fft_size), (2 * shift, 2)))


def edge_rows(plan):
    """rows of P[0..F), E whose decision sits exactly on a limit, with the record each must get"""
    f = plan["F"]
    up = lambda v: np.nextafter(F32(v), F32(np.inf))
    down = lambda v: np.nextafter(F32(v), F32(0))
    big = F32(2.0 ** 40)
    sr, ms, hw, mp = (F32(plan[k]) for k in ("second_ratio", "min_share", "half_w", "min_power"))
    rows = []

    def row(at, E=0.0):
        q = np.zeros(f + 1, np.float32)
        for k, v in at.items():
            q[k] = v
        q[f] = E
        return q
    hz = lambda c: _hz(plan, [F32(1) if i == c else F32(0) for i in range(f)], c)      # a lone bin: its centre frequency
    p, q2 = 5, f - 4
    rows.append((row({p: mp}), (hz(p), 0)))                              # exactly the floor
    rows.append((row({p: down(mp)}), (0, 0)))
    # the second component: P2 * second_ratio == P1 exactly makes a pair (not below), one ulp less a single tone
    p2 = F32(2.0 ** 40)
    p1 = F32(p2 * sr)
    rows.append((row({p: p1, q2: p2}), (hz(p), hz(q2))))
    rows.append((row({p: up(p1), q2: p2}), (hz(p), 0)))
    rows.append((row({q2: p1, p: p2}), (hz(p), hz(q2))))                # the stronger one above the weaker: still ascending
    # the share: S == min_share * (E * half_w) exactly is tonal, one ulp below is not
    e_tie = F32(2.0 ** 32)
    need = F32(ms * F32(e_tie * hw))
    rows.append((row({p: need}, E=e_tie), (hz(p), 0)))
    rows.append((row({p: down(need)}, E=e_tie), (0, 0)))
    # two equal maxima: the first is the peak, the other (three bins on) makes it a pair; two bins on it is a neighbour's neighbour
    rows.append((row({p: big, p + 3: big}), (hz(p), hz(p + 3))))
    rows.append((row({p: big, p + 2: big}), (hz(p), 0)))
    # both grid edges: the outer neighbour is 0
    rows.append((row({0: big}), (hz(0), 0)))
    rows.append((row({f - 1: big}), (hz(f - 1), 0)))
    rows.append((row({0: big, f - 1: big}), (hz(0), hz(f - 1))))
    # NaN: behind the peak it never wins a comparison; as the energy it never refuses
    nan = row({p: big})
    nan[p + 1] = np.nan
    rows.append((nan, None))                                             # (the record is whatever the statement gives: all sides alike)
    rows.append((row({p: big}, E=np.nan), (hz(p), 0)))
    rows.append((row({}), (0, 0)))                                       # silence
    out = []
    for qrow, want in rows:
        got = decide(plan, qrow)
        assert want is None or got == want, (qrow[:8], got, want)
        out.append((qrow, got))
    return out


# ------------------------------------------------------------------ signals
def to_pcm(sig):
    return np.clip(np.round(np.asarray(sig) * 32768.0), -32768, 32767).astype(np.int16)


def sine(hz, n, rate, level_dbfs=-12.0, phase=0.3):
    return 10.0 ** (level_dbfs / 20.0) * np.sin(2 * np.pi * hz * np.arange(n) / float(rate) + phase)


def pair(hz1, hz2, n, rate, level_dbfs=-15.0, twist_db=0.0):
    return sine(hz1, n, rate, level_dbfs, 0.3) + sine(hz2, n, rate, level_dbfs + twist_db, 1.1)


def noise(n, level_dbfs, seed):
    return np.random.RandomState(seed).normal(0.0, 10.0 ** (level_dbfs / 20.0), size=n)


def voice_like(n, rate, seed):
    """a harmonic voice-like signal: a pitch that glides between 90 and 220 Hz, twenty harmonics under a formant-like envelope"""
    rng = np.random.RandomState(seed)
    t = np.arange(n) / float(rate)
    f0 = 150.0 + 60.0 * np.sin(2 * np.pi * 1.3 * t + rng.uniform(0, 6)) + 10.0 * np.sin(2 * np.pi * 5.1 * t)
    ph = 2 * np.pi * np.cumsum(f0) / rate
    sig = np.zeros(n)
    for h in range(1, 21):
        fh = h * 150.0
        env = np.exp(-((fh - 600.0) / 500.0) ** 2) + 0.6 * np.exp(-((fh - 1500.0) / 500.0) ** 2) + 0.05
        sig += env * np.sin(h * ph + rng.uniform(0, 6))
    return 0.2 * sig / np.abs(sig).max() + noise(n, -50.0, seed + 1)


def sequence(items, rate, noise_dbfs=-60.0, seed=0):
    """int16 PCM of a tone sequence: items are ((hz, ...) or None for a pause, milliseconds); and the (start_ms, end_ms) of every tone"""
    parts, edges, at = [], [], 0
    for hz, ms in items:
        n = rate * ms // 1000
        if hz is None:
            parts.append(np.zeros(n))
        else:
            parts.append(sine(hz[0], n, rate, -12.0) if len(hz) == 1 else pair(hz[0], hz[1], n, rate, -15.0))
            edges.append((at, at + ms))
        at += ms
    sig = np.concatenate(parts)
    return to_pcm(sig + noise(len(sig), noise_dbfs, seed)), edges


# the issue's event scenario: 1100 Hz for 500 ms, silence for 200 ms, 480 + 620 Hz 500 ms on / 500 ms off twice, a 1400 Hz beep of 150 ms
SCENARIO = [(None, 100), ((1100,), 500), (None, 200), ((480, 620), 500), (None, 500), ((480, 620), 500), (None, 500), ((1400,), 150), (None, 300)]
SCENARIO_NAMES = ["cng", "busy", "busy", "sit2"]
