"""The DTMF contract stated in numpy: options -> plan, tables, steps 1-5 per frame, and the event machine.
Written from the text of the contract, not from csrc/dtmf.h; the CPU and GPU tests hold the product against it on every bit.
All fp32 arithmetic is spelled with np.float32 operands, one operation per statement, so nothing is contracted or widened."""
import numpy as np

F = np.float32
HZ = (697, 770, 852, 941, 1209, 1336, 1477, 1633)
DIGITS = "123A456B789C*0#D"
DOWN, UP = 1, 2
DEFAULTS = dict(min_level_dbfs=-40.0, twist_hi_db=4.0, twist_lo_db=8.0, rel_peak_db=8.0, min_share=0.6, min_tone_ms=20, min_pause_ms=20)


def options(**kw):
    d = dict(DEFAULTS)
    d.update(kw)
    return d


def window(rate, fft_size):
    """Wd = min(fft_size, 64 floor(0.016 rate / 64)) -- 0.016 rate / 64 is rate / 4000 --, or None for a refused model"""
    if rate < 4000 or fft_size <= 0:
        return None
    wd = min(int(fft_size), 64 * (int(rate) // 4000))
    if wd * 1000 < 12 * rate or wd > 4096:
        return None
    return wd


def options_valid(o):
    f = [o["min_level_dbfs"], o["twist_hi_db"], o["twist_lo_db"], o["rel_peak_db"], o["min_share"]]
    if not all(np.isfinite(F(v)) for v in f):
        return False
    return bool(-70 <= F(o["min_level_dbfs"]) <= 0 and 0 <= F(o["twist_hi_db"]) <= 20 and 0 <= F(o["twist_lo_db"]) <= 20
                and 3 <= F(o["rel_peak_db"]) <= 30 and 0 < F(o["min_share"]) <= 1
                and 10 <= o["min_tone_ms"] <= 1000 and 10 <= o["min_pause_ms"] <= 1000)


def make_plan(rate, fft_size, shift_ms, o):
    wd = window(rate, fft_size)
    if wd is None or shift_ms <= 0 or not options_valid(o):
        return None
    db = lambda v: float(F(v))                        # the option as the fp32 the C struct holds
    amp = 32768.0 * 10.0 ** (db(o["min_level_dbfs"]) / 20.0) * wd / 2.0
    return dict(Wd=wd, half_w=F(0.5) * F(wd), min_power=F(amp * amp), twist_hi=F(10.0 ** (db(o["twist_hi_db"]) / 10.0)),
                twist_lo=F(10.0 ** (db(o["twist_lo_db"]) / 10.0)), rel_peak=F(10.0 ** (db(o["rel_peak_db"]) / 10.0)), min_share=F(o["min_share"]),
                on_frames=max(1, int(o["min_tone_ms"]) // shift_ms), off_frames=max(1, int(o["min_pause_ms"]) // shift_ms))


def tables_f64(rate, wd):
    """[16][Wd] in double: rows 0..7 cos, rows 8..15 sin of 2 pi f_k j / rate"""
    j = np.arange(wd, dtype=np.float64)
    w = np.array([2.0 * np.pi * f * j / rate for f in HZ])
    return np.concatenate([np.cos(w), np.sin(w)])


def powers(plan, tables, frames):
    """steps 1 and 2: frames [n][>= Wd] int16, tables [16][Wd] float32 -> [n][9] float32: P[0..8), E"""
    wd = plan["Wd"]
    x = np.asarray(frames)[:, :wd]
    xf = x.astype(np.float32)
    t = np.asarray(tables, np.float32)
    assert t.shape == (16, wd)
    m = xf[:, None, :] * t[None, :, :]                # [n][16][Wd], fp32 products
    a = np.zeros((len(x), 16, 64), np.float32)
    for k in range(0, wd, 64):
        seg = m[:, :, k:k + 64]
        a[:, :, :seg.shape[2]] = a[:, :, :seg.shape[2]] + seg
    idx = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        a = a + a[:, :, idx ^ d]
    c = a[:, :, 0]
    re, im = c[:, :8], c[:, 8:]
    rr = re * re
    ii = im * im
    out = np.zeros((len(x), 9), np.float32)
    out[:, :8] = rr + ii
    e = (x.astype(np.int64) ** 2).sum(axis=1)
    out[:, 8] = e.astype(np.float32)
    assert a.dtype == np.float32 and out.dtype == np.float32
    return out


def decide(plan, q):
    """steps 3 and 4 on one row of P[0..8), E"""
    P = [F(v) for v in q[:8]]
    E = F(q[8])
    r = c = 0
    for i in range(1, 4):
        if P[i] > P[r]:
            r = i
        if P[4 + i] > P[4 + c]:
            c = i
    pr, pc = P[r], P[4 + c]
    with np.errstate(all="ignore"):
        if not (pr >= plan["min_power"] and pc >= plan["min_power"]):
            return 0
        if pc > F(pr * plan["twist_hi"]) or pr > F(pc * plan["twist_lo"]):
            return 0
        for i in range(4):
            if i != r and F(P[i] * plan["rel_peak"]) > pr:
                return 0
            if i != c and F(P[4 + i] * plan["rel_peak"]) > pc:
                return 0
        if F(pr + pc) < F(plan["min_share"] * F(E * plan["half_w"])):
            return 0
    return 1 + 4 * r + c


def run(plan, tables, frames):
    """(codes [n] uint8, powers [n][9])"""
    q = powers(plan, tables, frames)
    return np.array([decide(plan, row) for row in q], np.uint8), q


def machine():
    return dict(held=0, cand=0, run=0)


def events(plan, shift_ms, t0, codes, m):
    """the event machine over the codes of frames t0 .. ; m is updated in place.  [(kind, digit, time_ms)]"""
    on, off = plan["on_frames"], plan["off_frames"]
    out = []
    for i, c in enumerate(int(v) for v in codes):
        t = t0 + i
        if m["held"]:
            m["run"] = m["run"] + 1 if c != m["held"] else 0
            if m["run"] < off:
                continue
            out.append((UP, DIGITS[m["held"] - 1], (t - off + 1) * shift_ms))
            m.update(held=0, cand=0, run=0)           # ... and this frame starts the next candidate run
        if c != m["cand"]:
            m.update(cand=c, run=1 if c else 0)
        elif c:
            m["run"] += 1
        if c and m["run"] >= on:
            out.append((DOWN, DIGITS[c - 1], (t - on + 1) * shift_ms))
            m.update(held=c, cand=0, run=0)
    return out


def flush(shift_ms, frames_seen, m):
    out = [(UP, DIGITS[m["held"] - 1], frames_seen * shift_ms)] if m["held"] else []
    m.update(held=0, cand=0, run=0)
    return out


def frames_of(pcm, fft_size, shift):
    """frame t = pcm[t shift : t shift + fft_size], every whole frame, as a contiguous [n][fft_size] int16 array"""
    pcm = np.asarray(pcm, np.int16)
    n = (len(pcm) - fft_size) // shift + 1 if len(pcm) >= fft_size else 0
    if n <= 0:
        return np.zeros((0, fft_size), np.int16)
    return np.ascontiguousarray(np.lib.stride_tricks.as_strided(pcm, (n, fft_size), (2 * shift, 2)))


def tie_rows(plan):
    """rows of P[0..8), E whose decision sits exactly on a limit, with the code each must get; pr, pc far above min_power"""
    big = F(2.0 ** 40)
    up = lambda v: np.nextafter(F(v), F(np.inf))
    rows = []

    def row(pr, pc, other_r=0.0, other_c=0.0, E=0.0, r=1, c=2):
        q = np.zeros(9, np.float32)
        q[:4] = other_r
        q[4:8] = other_c
        q[r] = pr
        q[4 + c] = pc
        q[8] = E
        return q
    code = 1 + 4 * 1 + 2
    th, tl, rp, ms, hw = (F(plan[k]) for k in ("twist_hi", "twist_lo", "rel_peak", "min_share", "half_w"))
    rows.append((row(big, F(big * th)), code))                    # pc == pr * twist_hi: not above it
    rows.append((row(big, up(big * th)), 0))
    rows.append((row(F(big * tl), big), code))                    # pr == pc * twist_lo
    rows.append((row(up(big * tl), big), 0))
    rows.append((row(F(big * rp), F(big * rp), other_r=big), code))      # P[i] * rel_peak == pr for every other row
    rows.append((row(F(big * rp), F(big * rp), other_r=up(big)), 0))
    rows.append((row(F(big * rp), F(big * rp), other_c=big), code))
    rows.append((row(F(big * rp), F(big * rp), other_c=up(big)), 0))
    e_tie = F(2.0 ** 32)                                          # pr + pc == min_share * (E * half_w): both halves of the right side, exactly
    half = F(F(ms * F(e_tie * hw)) * F(0.5))
    rows.append((row(half, half, E=e_tie), code))
    rows.append((row(np.nextafter(half, F(0)), np.nextafter(half, F(0)), E=e_tie), 0))
    rows.append((row(F(plan["min_power"]), F(plan["min_power"])), code))       # exactly the floor
    rows.append((row(np.nextafter(F(plan["min_power"]), F(0)), F(plan["min_power"])), 0))
    two = row(big, big, r=0)                                      # two equal row peaks: the first is the peak -- and the other one refuses it
    two[2] = big
    rows.append((two, 0))
    two_floor = row(big, big, r=1)                                # ... equal peaks in rows 1 and 3, the other rows empty: still refused, by row 3
    two_floor[3] = big
    rows.append((two_floor, 0))
    nan = row(big, big)
    nan[3] = np.nan                                               # a NaN behind the peak: every comparison with it is false, the digit stands
    rows.append((nan, code))
    nan_e = row(big, big, E=np.nan)
    rows.append((nan_e, code))
    return rows


# ------------------------------------------------------------------ signals
STRING = "1122" + DIGITS + "00##DD"


def tone(digit, n, rate, level_dbfs=-12.0, twist_db=0.0, phase=(0.3, 1.1)):
    """n samples (float, full scale 1.0) of a digit: the row tone at level_dbfs, the column tone twist_db above it"""
    k = DIGITS.index(digit)
    t = np.arange(n) / float(rate)
    a = 10.0 ** (level_dbfs / 20.0)
    return a * np.sin(2 * np.pi * HZ[k // 4] * t + phase[0]) + a * 10.0 ** (twist_db / 20.0) * np.sin(2 * np.pi * HZ[4 + k % 4] * t + phase[1])


def digit_signal(digits, tone_ms, pause_ms, rate=16000, noise_dbfs=-50.0, lead_samples=0, seed=0, level_dbfs=-12.0, tail_ms=200):
    """int16 PCM: lead_samples + 100 ms of noise, then every digit for tone_ms followed by pause_ms of noise, then tail_ms; and the
    onset (sample index) of every digit"""
    rng = np.random.RandomState(seed)
    nt, npause = rate * tone_ms // 1000, rate * pause_ms // 1000
    parts, onsets, at = [np.zeros(lead_samples + rate // 10)], [], lead_samples + rate // 10
    for d in digits:
        onsets.append(at)
        parts += [tone(d, nt, rate, level_dbfs), np.zeros(npause)]
        at += nt + npause
    parts.append(np.zeros(rate * tail_ms // 1000))
    sig = np.concatenate(parts)
    sig = sig + rng.normal(0.0, 10.0 ** (noise_dbfs / 20.0), size=len(sig))
    return np.clip(np.round(sig * 32768.0), -32768, 32767).astype(np.int16), onsets


def digits_of(ev):
    return "".join(d for k, d, _ in ev if k == DOWN)


def keys_signal(items, rate=16000, noise_dbfs=-50.0, seed=0, level_dbfs=-12.0):
    """int16 PCM of a key sequence: items are (digit or None for a pause, milliseconds); and the onset in ms of every digit"""
    rng = np.random.RandomState(seed)
    parts, onsets, at = [], [], 0
    for d, ms in items:
        n = rate * ms // 1000
        if d is not None:
            onsets.append(at)
        parts.append(np.zeros(n) if d is None else tone(d, n, rate, level_dbfs))
        at += ms
    sig = np.concatenate(parts)
    sig = sig + rng.normal(0.0, 10.0 ** (noise_dbfs / 20.0), size=len(sig))
    return np.clip(np.round(sig * 32768.0), -32768, 32767).astype(np.int16), onsets
