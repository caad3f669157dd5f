"""Line quality (csrc/quality.h) on the CPU: the host statement of the contract (aprilx_quality_host,
aprilx_quality_events_host) against the numpy statement (tests/quality_ref.py) on every word, the clip runs at their edges, the event
machine against hand-derived sequences, every option at both ends of its range, the refusals, and the header alone under the sanitizers
as a stand-alone program (tests/cpp/quality_test.cc)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import quality_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "april_asr_amd", "csrc")
SH = 10                                           # frame shift in ms throughout
HOPS = (80, 160, 480)


def A():
    import april_asr_amd
    return april_asr_amd


def plan_dict(p):
    return {n: int(getattr(p, n)) for n in ("hop", "clip_level", "clip_run_min", "hold_frames", "dropout_frames", "report_frames")}


def inputs(hop, seed=0):
    """[name, frames [n][hop + 7]]: the hop is the first `hop` samples of a longer frame, as in the engine; what lies behind it must
    not count"""
    rng = np.random.RandomState(seed)
    ld = hop + 7

    def frame(x):
        f = rng.randint(-32768, 32768, size=ld).astype(np.int16)
        f[:hop] = x
        return f
    alt = np.where(np.arange(hop) % 2 == 0, 32767, -32767).astype(np.int16)
    return [("random", np.stack([frame(rng.randint(-32768, 32768, size=hop)) for _ in range(6)])),
            ("quiet", np.stack([frame(rng.randint(-30, 31, size=hop)) for _ in range(3)])),
            ("zeros", frame(np.zeros(hop, np.int16))[None]), ("stuck", frame(np.full(hop, 1234, np.int16))[None]),
            ("lowest", frame(np.full(hop, -32768, np.int16))[None]), ("alternating", frame(alt)[None])]


@pytest.mark.parametrize("hop", HOPS)
def test_host_equals_numpy_on_every_word(built, hop):
    for name, fr in inputs(hop):
        for level in (32767, 32124, 1024):
            got, want = A().quality_host(hop, level, fr), R.run(hop, level, fr)
            assert got.tolist() == want.tolist(), (name, level)
    # what the words must hold, by hand: all -32768 gives sumsq = H 2^30 (past 32 bits from H = 4 on), sum = -H 2^15, min = max = 0x8000
    w = [int(x) for x in A().quality_host(hop, 32767, np.full((1, hop), -32768, np.int16))[0]]
    assert w[0] | w[1] << 32 == hop << 30 and w[1] > 0 and w[2] == (-hop * 32768) & 0xffffffff
    assert w[3] == 0x80008000 and w[4] == hop | hop << 16 and w[5:] == [1, 0, 0]
    w = [int(x) for x in A().quality_host(hop, 32767, np.full((1, hop), 1234, np.int16))[0]]
    assert w == [hop * 1234 * 1234 & 0xffffffff, hop * 1234 * 1234 >> 32, hop * 1234, 1234 | 1234 << 16, 0, 1, 0, 0]
    alt = np.where(np.arange(hop) % 2 == 0, 32767, -32767).astype(np.int16)[None]
    w = [int(x) for x in A().quality_host(hop, 32767, alt)[0]]
    assert w[2] == 0 and w[3] == (32767 << 16 | (-32767 & 0xffff)) and w[4] == hop | hop << 16 and w[5] == 0


def run_word(hop, level, x):
    w = A().quality_host(hop, level, np.asarray(x, np.int16)[None])
    assert w.tolist() == R.run(hop, level, np.asarray(x, np.int16)[None]).tolist()
    return int(w[0][4]) & 0xffff, int(w[0][4]) >> 16


@pytest.mark.parametrize("hop", HOPS)
def test_clip_runs_at_their_edges(built, hop):
    L = 32124
    base = np.zeros(hop, np.int16)

    def with_run(at, n, value=L):
        x = base.copy()
        x[at:at + n] = value
        return x
    assert run_word(hop, L, with_run(5, 2)) == (2, 2)                 # clip_run_min - 1 for the default 3 ...
    assert run_word(hop, L, with_run(5, 3)) == (3, 3)                 # ... and exactly clip_run_min
    assert run_word(hop, L, with_run(61, 6)) == (6, 6)                # straddles samples 63 | 64
    assert run_word(hop, L, with_run(0, hop)) == (hop, hop)           # every slab full
    assert run_word(hop, L, with_run(hop - 2, 2)) == (2, 2)           # ends at H - 1
    assert run_word(hop, L, with_run(5, 3, L - 1)) == (0, 0)          # x = L - 1 is not clipped ...
    assert run_word(hop, L, with_run(5, 3, -L)) == (3, 3)             # ... x = -L is
    assert run_word(hop, L, with_run(5, 3, -L + 1)) == (0, 0)
    x = with_run(3, 4)
    x[10:12] = -L
    x[12:15] = 32767
    assert run_word(hop, L, x) == (9, 5)                              # two runs: the count adds, the run is the longer one; signs mix
    # a run of five across the hop boundary counts as two shorter runs: three at the end of one hop, two at the start of the next
    pcm = np.zeros(2 * hop, np.int16)
    pcm[hop - 3:hop + 2] = L
    rec = A().quality_host(hop, L, pcm.reshape(2, hop))
    assert [(int(w[4]) & 0xffff, int(w[4]) >> 16) for w in rec] == [(3, 3), (2, 2)]
    assert rec.tolist() == R.run(hop, L, pcm.reshape(2, hop)).tolist()


def synth(hop, spec, level=32767):
    """records of a sequence of frames given as a string: 'c' clipped (a run of 3 at the level), 'd' dead (zeros), 's' stuck at 77,
    '.' live and unclipped"""
    rng = np.random.RandomState(5)
    rows = []
    for ch in spec:
        x = rng.randint(-2000, 2001, size=hop).astype(np.int16)
        if ch == "c":
            x[7:10] = level
        elif ch == "d":
            x[:] = 0
        elif ch == "s":
            x[:] = 77
        rows.append(x)
    return np.stack(rows)


def both(opts, spec, hop=160, t0=0, flush=False, cuts=()):
    """the events of the library's machine and of the numpy statement over the same records (cut at `cuts`, the machine carried)"""
    o = R.options(**opts)
    plan = A().quality_plan(16000 * hop // 160, 3 * hop, SH, opts or True)
    p = R.make_plan(16000 * hop // 160, 3 * hop, SH, o)
    assert plan_dict(plan) == p
    rec = R.run(hop, o["clip_level"], synth(hop, spec, o["clip_level"]))
    got, want, m, rm = [], [], None, R.machine()
    edges = [0] + list(cuts) + [len(rec)]
    for k, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        last = flush and k == len(edges) - 2
        ev, m = A().quality_events_host(plan, SH, t0 + a, rec[a:b], m, flush=last)
        got += [e.astuple() for e in ev]
        want += R.events(p, SH, t0 + a, rec[a:b], rm) + (R.flush(p, SH, t0 + b, rm) if last else [])
    assert got == want, (got, want)
    return [(e[0], e[2]) for e in got if e[0] != R.REPORT], [e for e in got if e[0] == R.REPORT]


def test_clipping_on_at_the_first_clipped_frame_and_off_exactly_after_the_hold(built):
    opts = dict(clip_hold_ms=100, report_ms=0)                        # hold: 10 frames
    ev, _ = both(opts, "..c" + "." * 10)
    assert ev == [(R.CLIPPING_ON, 20), (R.CLIPPING_OFF, 30)]          # OFF at the first of the ten unclipped frames
    ev, _ = both(opts, "..c" + "." * 9)
    assert ev == [(R.CLIPPING_ON, 20)]                                # ... and not one frame earlier
    ev, _ = both(opts, "..c" + "." * 9 + "c" + "." * 10)
    assert ev == [(R.CLIPPING_ON, 20), (R.CLIPPING_OFF, 130)]         # a clipped frame inside the hold starts it again
    ev, _ = both(opts, "c" + "." * 10 + "c", t0=1000, cuts=(1, 5, 11))
    assert ev == [(R.CLIPPING_ON, 10000), (R.CLIPPING_OFF, 10010), (R.CLIPPING_ON, 10110)]
    ev, _ = both(dict(clip_run_min=4, report_ms=0), "c" * 5)
    assert ev == []                                                   # a run of three is below clip_run_min 4


def test_dropout_needs_its_full_length(built):
    opts = dict(dropout_ms=200, report_ms=0)                          # 20 frames
    ev, _ = both(opts, ".." + "d" * 19 + "..")
    assert ev == []                                                   # dropout_ms - shift_ms of dead frames: no event
    ev, _ = both(opts, ".." + "d" * 20 + "dd..")
    assert ev == [(R.DROPOUT_ON, 20), (R.DROPOUT_OFF, 240)]
    ev, _ = both(opts, ".." + "d" * 10 + "s" * 10 + ".", cuts=(7, 21))
    assert ev == [(R.DROPOUT_ON, 20), (R.DROPOUT_OFF, 220)]           # a stuck value is dead too, and dead frames need not be alike
    ev, _ = both(opts, "d" * 19 + "." + "d" * 19 + ".")
    assert ev == []                                                   # a live frame starts the count again


def test_reports_and_the_flush(built):
    opts = dict(report_ms=100, clip_hold_ms=150, dropout_ms=20)
    spec = "." * 10 + "cc" + "." * 6 + "dd" + "." * 3
    ev, rep = both(opts, spec, flush=True, cuts=(4, 10, 19))
    fr = {n: i for i, n in enumerate(R.FIELDS)}
    assert [(r[fr["time_ms"]], r[fr["frames"]]) for r in rep] == [(0, 10), (100, 10), (200, 3)]      # the flush cuts the third interval short
    assert [r[fr["clipped_frames"]] for r in rep] == [0, 2, 0] and [r[fr["dead_frames"]] for r in rep] == [0, 2, 0]
    assert rep[1][fr["clip_samples"]] == 6 and rep[1][fr["max"]] == 32767 and rep[1][fr["quiet_sumsq"]] > 0
    assert ev == [(R.CLIPPING_ON, 100), (R.DROPOUT_ON, 180), (R.DROPOUT_OFF, 200), (R.CLIPPING_OFF, 230)]      # the hold had not passed: closed by the flush at frames_seen
    # an interval of dead frames only: quiet_sumsq is 0 (no live frame), loud_sumsq the stuck value's
    _, rep = both(dict(report_ms=100), "s" * 10)
    assert rep[0][fr["quiet_sumsq"]] == 0 and rep[0][fr["loud_sumsq"]] == 160 * 77 * 77 and rep[0][fr["dead_frames"]] == 10
    # a dropout that is on when the flush completes; the machine starts afresh behind it
    ev, rep = both(dict(report_ms=0, dropout_ms=20), "..ddd", flush=True)
    assert ev == [(R.DROPOUT_ON, 20), (R.DROPOUT_OFF, 50)] and rep == []
    plan = A().quality_plan(16000, 512, SH, dict(report_ms=100))
    rec = R.run(160, 32767, synth(160, "...."))
    _, m = A().quality_events_host(plan, SH, 0, rec, None, flush=True)
    assert bytes(m) == bytes(C.sizeof(m))
    ev, _ = A().quality_events_host(plan, SH, 4, rec, m, flush=True)
    assert [(e.time_ms, e.frames) for e in ev] == [(40, 4)]           # the next interval starts at the first frame behind the flush


def test_derived_levels(built):
    E = A().QualityEvent
    e = E(kind=1, frames=10, hop=160, sumsq=1600 * 16384 ** 2, sum=1600 * 100, min=-16384, max=8192, loud_sumsq=1000000, quiet_sumsq=1000)
    assert abs(e.rms_dbfs - 20 * np.log10(0.5)) < 1e-9 and abs(e.peak_dbfs - 20 * np.log10(0.5)) < 1e-9 and e.dc == 100.0 and abs(e.snr_db - 30.0) < 1e-9
    z = E(kind=1, frames=10, hop=160)
    assert z.rms_dbfs is None and z.peak_dbfs is None and z.snr_db is None and z.dc == 0.0


def test_every_option_at_both_ends_of_its_range_and_the_refusals(built):
    from april_asr_amd import _ffi
    L = _ffi.lib()

    def raw(size=None, flags=0, rate=16000, frame=512, shift=SH, **kw):
        d = R.options(**kw)
        o = _ffi.AprilxQualityOptions(C.sizeof(_ffi.AprilxQualityOptions) if size is None else size, flags, *[d[n] for n in A()._QUALITY_FIELDS])
        plan = _ffi.AprilxQualityPlan()
        rc = int(L.aprilx_quality_plan(rate, frame, shift, C.byref(o), C.byref(plan)))
        want = R.make_plan(rate, frame, shift, d) if size is None and not flags else None
        assert (rc == 0) == (want is not None), (kw, rc)
        if rc == 0:
            assert plan_dict(plan) == want, kw
        return rc
    assert C.sizeof(_ffi.AprilxQualityOptions) == 28 and C.sizeof(_ffi.AprilxQualityEvent) == 80 and C.sizeof(_ffi.AprilxQualityMachine) == 88
    assert raw() == 0
    for name, (lo, hi) in R.RANGES.items():
        assert [raw(**{name: v}) for v in (lo, hi, lo - 1, hi + 1)] == [0, 0, -1, -1], name
    assert raw(report_ms=0) == 0 and raw(report_ms=99) == -1 and raw(clip_level=0) == -1 and raw(clip_run_min=0) == -1
    assert raw(size=24) == -1 and raw(flags=1) == -1
    assert raw(rate=8000, frame=256) == 0 and raw(rate=48000, frame=2048) == 0
    assert raw(rate=16000, frame=100) == -1                           # a hop longer than the frame
    assert raw(shift=0) == -1 and raw(rate=0) == -1
    assert int(L.aprilx_quality_plan(16000, 512, SH, None, C.byref(_ffi.AprilxQualityPlan()))) == -1
    # the durations in frames at the ends
    assert plan_dict(A().quality_plan(16000, 512, SH, dict(clip_hold_ms=60000, dropout_ms=20, report_ms=60000))) == dict(
        hop=160, clip_level=32767, clip_run_min=3, hold_frames=6000, dropout_frames=2, report_frames=6000)
    # aprilx_quality_host and aprilx_quality_events_host
    fr = np.zeros((2, 160), np.int16); out = np.zeros((2, 8), np.uint32)

    def host(hop=160, level=32767, n=2, ld=160, frames=fr.ctypes.data, rec=out.ctypes.data):
        return int(L.aprilx_quality_host(hop, level, n, frames, ld, rec))
    assert [host(), host(n=0, frames=None, rec=None), host(hop=0), host(hop=32768), host(level=1023), host(level=32768), host(n=-1), host(ld=159),
            host(frames=None), host(rec=None)] == [0, 0, -1, -1, -1, -1, -1, -1, -1, -1]
    plan = A().quality_plan(16000, 512, SH)
    m = _ffi.AprilxQualityMachine()
    ev = (_ffi.AprilxQualityEvent * 4)()

    def events(plan_=plan, sh=SH, records=out.ctypes.data, n=2, machine=m, cap=4, out_=ev):
        return int(L.aprilx_quality_events_host(C.byref(plan_) if plan_ is not None else None, sh, 0, records, n, 0, C.byref(machine) if machine is not None else None,
                                                C.addressof(out_) if out_ is not None else None, cap))
    bad_plan = _ffi.AprilxQualityPlan(0, 32767, 3, 1, 1, 0)
    bad_m = _ffi.AprilxQualityMachine(); bad_m.clipping = 2
    assert [events(), events(plan_=None), events(plan_=bad_plan), events(sh=0), events(records=None), events(machine=None), events(machine=bad_m), events(cap=-1),
            events(out_=None), events(cap=0, out_=None)] == [0, -1, -1, -1, -1, -1, -1, -1, -1, 0]
    # more events than room: counted, not written
    rec = R.run(160, 32767, synth(160, "cc"))
    p1 = A().quality_plan(16000, 512, SH, dict(report_ms=100, clip_hold_ms=100))
    one = (_ffi.AprilxQualityEvent * 1)()
    assert int(L.aprilx_quality_events_host(C.byref(p1), SH, 0, rec.ctypes.data, 2, 1, C.byref(_ffi.AprilxQualityMachine()), C.addressof(one), 1)) == 3
    assert one[0].kind == R.CLIPPING_ON


def test_events_of_random_records_equal_the_statement(built):
    rng = np.random.RandomState(3)
    for trial in range(6):
        spec = "".join(rng.choice(list("cds...."), p=[0.1, 0.15, 0.05, 0.175, 0.175, 0.175, 0.175]) for _ in range(400))
        spec = spec[:100] + "d" * 30 + spec[130:260] + "." * 20 + spec[280:]
        opts = dict(clip_hold_ms=int(rng.choice([100, 150, 300])), dropout_ms=int(rng.choice([20, 50, 250])), report_ms=int(rng.choice([0, 100, 370])),
                    clip_run_min=int(rng.choice([1, 3, 4])))
        cuts = sorted(set(int(c) for c in rng.randint(1, 399, size=12)))
        ev, rep = both(opts, spec, t0=int(rng.randint(0, 5000)), flush=True, cuts=cuts)
        assert len(ev) >= 2                                           # (the thirty dead frames alone give a dropout)


def test_header_alone_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "quality_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "quality_test.cc"), "-o", exe], timeout=600)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0 and "all checks passed" in out, out[-3000:]
