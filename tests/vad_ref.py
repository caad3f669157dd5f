"""The voice-activity contract (csrc/vad.h) stated in numpy float32, independent of the product's code: the plan
from a mel table, steps 1-9 over an array of rows, and the events that follow from the bytes.  Every operation is one IEEE binary32
operation in the order the contract writes it; min and max are the comparisons vmin(a, b) = b if b < a else a and
vmax(a, b) = b if a < b else a.  `mut` names ONE deliberate change of a comparison or a constant: the hand-derived cases
(tests/golden/vad_cases.py) must each fail under theirs."""
import numpy as np

F = np.float32
ALPHA = F(0.25)
DB = F(0.23025851)
INF = F(np.inf)
SUB, WINDOWS, LANES = 32, 8, 16
START, END = 1, 2
DEFAULTS = dict(band_lo_hz=200.0, band_hi_hz=4000.0, onset_db=5.0, offset_db=3.0, onset_ms=50, hangover_ms=300, min_energy=-12.0)


def options(**kw):
    d = dict(DEFAULTS)
    d.update(kw)
    return d


def options_valid(o, rate):
    lo, hi, on, off = F(o["band_lo_hz"]), F(o["band_hi_hz"]), F(o["onset_db"]), F(o["offset_db"])
    if not (np.isfinite(lo) and np.isfinite(hi) and 0 <= lo < hi and float(hi) <= rate / 2):
        return False
    if not (np.isfinite(on) and np.isfinite(off) and 0 < off <= on <= 60):
        return False
    if not (10 <= o["onset_ms"] <= 1000 and 10 <= o["hangover_ms"] <= 10000):
        return False
    return bool(np.isfinite(F(o["min_energy"])))


def make_plan(mel, rate, shift_ms, o):
    """dict(b0, b1, inv_nb, thr_on, thr_off, min_energy, onset_frames, hangover_frames), or None when refused"""
    mel = np.asarray(mel, np.float32)
    if not options_valid(o, rate):
        return None
    nfft = mel.shape[1]
    peaks = np.argmax(mel, axis=1).astype(np.float64) * rate / (2.0 * nfft)       # (argmax: the first maximum)
    inside = (peaks >= float(F(o["band_lo_hz"]))) & (peaks <= float(F(o["band_hi_hz"])))
    if not inside.any():
        return None
    b0 = int(np.argmax(inside))
    b1 = b0
    while b1 < len(inside) and inside[b1]:
        b1 += 1
    return dict(b0=b0, b1=b1, inv_nb=F(1.0) / F(b1 - b0), thr_on=F(o["onset_db"]) * DB, thr_off=F(o["offset_db"]) * DB,
                min_energy=F(o["min_energy"]), onset_frames=max(1, int(o["onset_ms"]) // shift_ms), hangover_frames=max(1, int(o["hangover_ms"]) // shift_ms))


def reset_state():
    return dict(s=F(0), cur=INF, hist=[INF] * WINDOWS, cnt=0, pos=0, st=0, run=0, first=1)


def band_energy(plan, rows):
    """step 1 for every row at once: [n] float32"""
    x = np.asarray(rows, np.float32)
    x = x.reshape(len(x), -1)
    b0, b1 = plan["b0"], plan["b1"]
    c = np.zeros((len(x), LANES), np.float32)
    k = 0
    while b0 + LANES * k < b1:
        for l in range(LANES):
            i = b0 + l + LANES * k
            if i < b1:
                c[:, l] = c[:, l] + x[:, i]
        k += 1
    for m in (8, 4, 2, 1):
        c = c + c[:, np.arange(LANES) ^ m]
    return (c[:, 0] * F(plan["inv_nb"])).astype(np.float32)


def vmin(a, b):
    return b if b < a else a


def vmax(a, b):
    return b if a < b else a


def step(plan, v, e, mut=None):
    """steps 2-9 on one energy; returns the byte"""
    e = F(e)
    if mut != "noclamp":
        e = vmax(e, F(plan["min_energy"]))
    if v["first"] and mut != "nofirst":
        v["s"] = e
    else:
        t = F(e - v["s"])
        t = F(ALPHA * t)
        v["s"] = F(v["s"] + t)
    v["first"] = 0
    v["cur"] = vmin(v["cur"], v["s"])
    v["cnt"] += 1
    n = v["cur"]
    for h in v["hist"]:
        n = vmin(n, h)
    d = F(v["s"] - n)
    thr = F(plan["thr_off"]) if v["st"] else F(plan["thr_on"])
    raw = int(d >= thr) if mut == "ge" else int(d > thr)
    windows = WINDOWS + 1 if mut == "win9" else WINDOWS
    if len(v["hist"]) < windows:
        v["hist"] = v["hist"] + [INF] * (windows - len(v["hist"]))
    if v["cnt"] == (SUB + 1 if mut == "sub33" else SUB):
        v["hist"][v["pos"]] = v["cur"]
        v["pos"] = (v["pos"] + 1) % windows
        v["cur"] = INF
        v["cnt"] = 0
    if not v["st"]:
        v["run"] = v["run"] + 1 if raw else 0
        if v["run"] >= plan["onset_frames"] + (1 if mut == "onset_late" else 0):
            v["st"], v["run"] = 1, 0
    else:
        v["run"] = 0 if raw else v["run"] + 1
        if v["run"] >= plan["hangover_frames"] + (1 if mut == "hang_late" else 0):
            v["st"], v["run"] = 0, 0
    return v["st"] | raw << 1


def run(plan, rows, state=None, mut=None):
    """(bytes uint8 [n], energies float32 [n], state): rows through steps 1-9 from `state` (None: reset)"""
    v = reset_state() if state is None else state
    e = band_energy(plan, rows)
    b = np.array([step(plan, v, x, mut) for x in e], np.uint8)
    return b, e, v


def events(plan, shift_ms, t0, data, last=0):
    """([(kind, time_ms)], last bit) from bit 0 of the bytes of frames [t0, t0 + n)"""
    out = []
    for i, x in enumerate(np.asarray(data, np.uint8)):
        st, t = int(x) & 1, t0 + i
        if st and not last:
            out.append((START, (t - plan["onset_frames"] + 1) * shift_ms))
        elif last and not st:
            out.append((END, (t - plan["hangover_frames"] + 1) * shift_ms))
        last = st
    return out, last


def flush_end(frames_seen, shift_ms, last):
    """a flush that completes: closes an open segment"""
    return [(END, frames_seen * shift_ms)] if last else []


def state_tuple(v):
    """comparable on every bit: the floats as their bit patterns"""
    fl = np.array([v["s"], v["cur"]] + list(v["hist"][:WINDOWS]), np.float32).view(np.uint32).tolist()
    return tuple(fl) + (v["cnt"], v["pos"], v["st"], v["run"], v["first"])


def burst_signal(seconds, bursts, noise_dbfs=-50.0, snr_db=20.0, seed=0, rate=16000):
    """The speech stand-in of DESIGN.md section 16: harmonics of 120 Hz under a 4 Hz envelope inside the (start, end) spans of
    `bursts` (seconds), over Gaussian noise at noise_dbfs; int16."""
    rng = np.random.RandomState(seed)
    n = int(seconds * rate)
    t = np.arange(n) / rate
    noise = rng.normal(0, 10 ** (noise_dbfs / 20), size=n)
    sp = np.zeros(n)
    for h in range(1, 26):
        sp += np.sin(2 * np.pi * 120 * h * t + rng.uniform(0, 6.28)) / h
    sp *= 0.5 * (1 + np.sin(2 * np.pi * 4 * t))
    sp *= 10 ** ((noise_dbfs + snr_db) / 20) / np.sqrt(np.mean(sp ** 2))
    gate = np.zeros(n)
    for a, b in bursts:
        gate[int(a * rate):int(b * rate)] = 1
    return np.clip((noise + sp * gate) * 32767, -32768, 32767).astype(np.int16)
