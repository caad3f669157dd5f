"""The line-quality contract stated in numpy and plain Python, independent of the product: the record of a hop,
the plan, and the machine that turns consecutive records into reports and ON / OFF events.  All integers; Python's are unbounded, so the
statement holds the widths explicitly where the record packs them."""
import numpy as np

REPORT, CLIPPING_ON, CLIPPING_OFF, DROPOUT_ON, DROPOUT_OFF = 1, 2, 3, 4, 5
WORDS = 8
FIELDS = ("kind", "frames", "time_ms", "sum", "sumsq", "min", "max", "clip_samples", "clipped_frames", "dead_frames", "quiet_sumsq", "loud_sumsq", "hop")
DEFAULTS = dict(clip_level=32767, clip_run_min=3, clip_hold_ms=1000, dropout_ms=200, report_ms=1000)
RANGES = dict(clip_level=(1024, 32767), clip_run_min=(1, 64), clip_hold_ms=(100, 60000), dropout_ms=(20, 60000), report_ms=(100, 60000))


def options(**kw):
    d = dict(DEFAULTS)
    d.update(kw)
    return d


def options_valid(o):
    for name, (lo, hi) in RANGES.items():
        if name == "report_ms" and o[name] == 0:
            continue
        if not lo <= o[name] <= hi:
            return False
    return True


def make_plan(sample_rate, frame_samples, shift_ms, o):
    """None: refused"""
    if sample_rate <= 0 or frame_samples <= 0 or shift_ms <= 0 or not options_valid(o):
        return None
    hop = shift_ms * sample_rate // 1000
    if not 1 <= hop <= min(frame_samples, 32767):
        return None
    return dict(hop=hop, clip_level=o["clip_level"], clip_run_min=o["clip_run_min"], hold_frames=max(1, o["clip_hold_ms"] // shift_ms),
                dropout_frames=max(1, o["dropout_ms"] // shift_ms), report_frames=max(1, o["report_ms"] // shift_ms) if o["report_ms"] else 0)


def longest_run(flags):
    best = run = 0
    for f in flags:
        run = run + 1 if f else 0
        best = max(best, run)
    return best


def record(x, level):
    """the eight uint32 of one hop x (int16)"""
    v = [int(s) for s in np.asarray(x, np.int16)]
    sumsq = sum(s * s for s in v)
    total = sum(v)
    mn, mx = min(v), max(v)
    flags = [s >= level or s <= -level for s in v]
    assert sumsq < 1 << 64 and -(1 << 31) <= total < 1 << 31 and sum(flags) < 1 << 16
    return [sumsq & 0xffffffff, sumsq >> 32, total & 0xffffffff, (mn & 0xffff) | (mx & 0xffff) << 16, sum(flags) | longest_run(flags) << 16,
            1 if mn == mx else 0, 0, 0]


def run(hop, level, frames):
    """frames [n][>= hop] int16 -> records [n][8] uint32"""
    f = np.asarray(frames, np.int16)
    return np.array([record(row[:hop], level) for row in f], np.uint32).reshape(-1, WORDS)


def frames_of(pcm, frame_samples, shift):
    """frame k of a stream: samples [k shift, k shift + frame_samples), every frame that fits"""
    pcm = np.asarray(pcm, np.int16)
    n = max(0, (len(pcm) - frame_samples) // shift + 1)
    return np.stack([pcm[k * shift:k * shift + frame_samples] for k in range(n)]) if n else np.zeros((0, frame_samples), np.int16)


def unpack(w):
    w = [int(x) for x in w]
    s16 = lambda u: u - 65536 if u >= 32768 else u                                # noqa: E731
    total = w[2] - (1 << 32) if w[2] >= 1 << 31 else w[2]
    return dict(sumsq=w[0] | w[1] << 32, sum=total, min=s16(w[3] & 0xffff), max=s16(w[3] >> 16), clip_count=w[4] & 0xffff, clip_run=w[4] >> 16, dead=w[5] & 1)


def machine():
    return dict(clipping=0, dropout=0, quiet_run=0, dead_run=0, interval=[], first=0)


def event(kind, time_ms, hop, **kw):
    e = dict.fromkeys(FIELDS, 0)
    e.update(kind=kind, time_ms=time_ms, hop=hop, **kw)
    return tuple(e[n] for n in FIELDS)


def report(p, sh, m):
    """the open interval (a list of unpacked records) as a REPORT, or nothing when it is empty; the interval is emptied"""
    iv = m["interval"]
    m["interval"] = []
    if not iv:
        return []
    live = [r["sumsq"] for r in iv if not r["dead"]]
    return [event(REPORT, m["first"] * sh, p["hop"], frames=len(iv), sum=sum(r["sum"] for r in iv), sumsq=sum(r["sumsq"] for r in iv), min=min(r["min"] for r in iv),
                  max=max(r["max"] for r in iv), clip_samples=sum(r["clip_count"] for r in iv),
                  clipped_frames=sum(r["clip_run"] >= p["clip_run_min"] for r in iv), dead_frames=sum(r["dead"] for r in iv),
                  quiet_sumsq=min(live) if live else 0, loud_sumsq=max(r["sumsq"] for r in iv))]


def events(p, sh, t0, records, m):
    """the events of frames [t0, t0 + n) as tuples in FIELDS order; per frame: clipping, dropout, report"""
    out = []
    for i, w in enumerate(np.asarray(records, np.uint32).reshape(-1, WORDS)):
        r, t = unpack(w), t0 + i
        clipped = r["clip_run"] >= p["clip_run_min"]
        if not m["clipping"]:
            if clipped:
                m["clipping"], m["quiet_run"] = 1, 0
                out.append(event(CLIPPING_ON, t * sh, p["hop"]))
        elif clipped:
            m["quiet_run"] = 0
        else:
            m["quiet_run"] += 1
            if m["quiet_run"] >= p["hold_frames"]:
                out.append(event(CLIPPING_OFF, (t - m["quiet_run"] + 1) * sh, p["hop"]))
                m["clipping"], m["quiet_run"] = 0, 0
        if r["dead"]:
            if not m["dropout"]:
                m["dead_run"] += 1
                if m["dead_run"] >= p["dropout_frames"]:
                    out.append(event(DROPOUT_ON, (t - m["dead_run"] + 1) * sh, p["hop"]))
                    m["dropout"], m["dead_run"] = 1, 0
        else:
            if m["dropout"]:
                m["dropout"] = 0
                out.append(event(DROPOUT_OFF, t * sh, p["hop"]))
            m["dead_run"] = 0
        if p["report_frames"]:
            if not m["interval"]:
                m["first"] = t
            m["interval"].append(r)
            if len(m["interval"]) >= p["report_frames"]:
                out += report(p, sh, m)
    return out


def flush(p, sh, t, m):
    """a flush completed behind frame t - 1: OFF of what is on at t * sh, the open interval as a short report, a fresh machine"""
    out = []
    if m["clipping"]:
        out.append(event(CLIPPING_OFF, t * sh, p["hop"]))
    if m["dropout"]:
        out.append(event(DROPOUT_OFF, t * sh, p["hop"]))
    out += report(p, sh, m)
    m.clear()
    m.update(machine())
    return out
