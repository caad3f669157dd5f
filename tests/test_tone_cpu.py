"""Tones without a GPU: the contract in plain C++ (aprilx_tone_plan, aprilx_tone_tables, aprilx_tone_host,
aprilx_tone_decide_host, aprilx_tone_events_host, aprilx_tone_name; csrc/tone.h) against its numpy statement (tests/tone_ref.py) on every
bit, the decision's exact ties, detection quality on seeded synthetic signals with the bounds section 18 records, the event scenario with
its times, every refusal, and the header and the staging layout's sixth array under AddressSanitizer + UBSan as stand-alone programs
(tests/cpp/tone_test.cc, tests/cpp/staging_layout_tone_test.cc).
Run as a script it prints the measured figures the assertions below were taken from."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import april_asr_amd as A
from april_asr_amd import _ffi
from conftest import speech_like_pcm
import tone_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "april_asr_amd", "csrc")
# (rate, fft_size, frame shift in samples): W 512, W 256, 400-sample frames that are not rounded up (W 384), and 48 kHz (W 2048, F 86)
GEOMETRIES = {"16k": (16000, 512, 160), "8k": (8000, 256, 80), "n400": (16000, 400, 160), "48k": (48000, 2048, 480)}
GRIDS = {"16k": (512, 10, 64), "8k": (256, 10, 64), "n400": (384, 8, 48), "48k": (2048, 13, 86)}


def plan_dict(p):
    return dict(W=p.W, k_lo=p.k_lo, F=p.F, half_w=R.F32(p.half_w), min_power=R.F32(p.min_power), second_ratio=R.F32(p.second_ratio),
                min_share=R.F32(p.min_share), bin_hz=R.F32(p.bin_hz), tol_hz=p.tol_hz, on_frames=p.on_frames, off_frames=p.off_frames)


def setup(geo, options=True):
    rate, fft, shift = GEOMETRIES[geo]
    plan = A.tone_plan(rate, fft, 10, options)
    return rate, fft, shift, plan, A.tone_tables(rate, fft)


def same_bits(a, b):
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def tup(ev):
    return [(e.kind, e.f1_hz, e.f2_hz, e.time_ms) for e in ev]


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_tables_and_plan(built, geo):
    rate, fft, shift, plan, t = setup(geo)
    assert (plan.W, plan.k_lo, plan.F) == R.grid(rate, fft) == GRIDS[geo]
    assert t.shape == (2 * plan.F, plan.W)
    assert np.abs(t.astype(np.float64) - R.tables_f64(plan.W, plan.k_lo, plan.F)).max() <= 1e-7
    want = R.make_plan(rate, fft, 10, R.options())
    got = plan_dict(plan)
    for k in ("W", "k_lo", "F", "on_frames", "off_frames", "tol_hz", "half_w", "min_share", "bin_hz"):
        assert got[k] == want[k], k
    for k in ("min_power", "second_ratio"):                                        # (pow() of two libms: within an ulp of fp32)
        assert abs(float(got[k]) - float(want[k])) <= 1.2e-7 * float(want[k]), k
    assert (got["on_frames"], got["off_frames"]) == (6, 3)


def signal_set(rate, plan, n):
    """single tones on a bin, midway between bins and at both grid edges, the two pairs, noise, and the tests' speech-like signal"""
    bin_hz = rate / float(plan.W)
    sigs = [("on_bin", R.sine((plan.k_lo + 20) * bin_hz, n, rate)), ("midway", R.sine((plan.k_lo + 20.5) * bin_hz, n, rate)),
            ("low_edge", R.sine(plan.k_lo * bin_hz, n, rate)), ("high_edge", R.sine((plan.k_lo + plan.F - 1) * bin_hz, n, rate, -6.0)),
            ("dial", R.pair(350, 440, n, rate)), ("busy", R.pair(480, 620, n, rate, twist_db=-4.0)), ("noise", R.noise(n, -20.0, 4))]
    out = [(name, R.to_pcm(sig + R.noise(n, -55.0, 9))) for name, sig in sigs]
    return out + [("speech", speech_like_pcm(n / 16000.0 + 0.1, seed=2)[:n])]


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_host_equals_numpy_on_every_bit(built, geo):
    rate, fft, shift, plan, t = setup(geo)
    p = plan_dict(plan)
    n = 23 * shift + fft
    tonal = {}
    for name, pcm in signal_set(rate, plan, n) + [("silence", np.zeros(n, np.int16)), ("lowest", np.full(n, -32768, np.int16))]:
        frames = R.frames_of(pcm, fft, shift)
        assert len(frames) == 24
        rec, pw = A.tone_host(plan, t, frames)
        want_r, want_p = R.run(p, t, frames)
        assert rec.tolist() == want_r.tolist(), (geo, name)
        assert same_bits(pw, want_p), (geo, name)
        tonal[name] = int((rec[:, 0] != 0).sum())
        if name in ("on_bin", "midway", "low_edge", "high_edge"):
            assert (rec[:, 0] != 0).all() and not rec[:, 1].any(), (geo, name, rec.tolist())
        if name == "busy" or (name == "dial" and geo != "n400"):                   # (41.7 Hz bins: 350 and 440 Hz lie closer than three bins)
            assert (rec[:, 0] != 0).all() and (rec[:, 1] != 0).all(), (geo, name, rec.tolist())
    assert tonal["noise"] == tonal["silence"] == tonal["lowest"] == 0
    assert float(pw[0, plan.F]) == float(plan.W) * 2.0 ** 30                        # the energy of W samples of -32768, exactly


def test_exact_ties_in_the_decision(built):
    for geo in sorted(GEOMETRIES):
        _, _, _, plan, _ = setup(geo)
        p = plan_dict(plan)
        rows = R.edge_rows(p)                                                       # (asserts the records the text promises)
        assert len(rows) >= 14
        for i, (q, want) in enumerate(rows):
            assert A.tone_decide_host(plan, q) == tuple(want), (geo, i)


# ------------------------------------------------------------------ detection quality (the figures of DESIGN.md section 18)
def measure_singles(geo, count=2000, seed=100):
    """`count` single tones at 330..2250 Hz, -30..-3 dBFS, random phase, white noise 25 dB below the tone, one frame each:
    (largest frequency error in Hz, smallest share, frames reported as a pair, frames not tonal)"""
    rate, fft, shift, plan, t = setup(geo)
    rng = np.random.RandomState(seed)
    hz = rng.uniform(330.0, 2250.0, count)
    lev = rng.uniform(-30.0, -3.0, count)
    frames = np.stack([R.to_pcm(R.sine(hz[i], fft, rate, lev[i], rng.uniform(0, 2 * np.pi)) + R.noise(fft, lev[i] - 3.0 - 25.0, seed + 1 + i))
                       for i in range(count)])      # (a sine's power is 3 dB below its peak level)
    rec, pw = A.tone_host(plan, t, frames)
    err = np.abs(rec[:, 0].astype(np.float64) - hz)
    F = plan.F
    shares = []
    for q in pw:
        c = int(np.argmax(q[:F]))
        s = float(q[max(0, c - 1):c + 2].astype(np.float64).sum())
        shares.append(s / (float(q[F]) * float(plan.half_w)))
    return float(err[rec[:, 0] != 0].max()), float(min(shares)), int((rec[:, 1] != 0).sum()), int((rec[:, 0] == 0).sum())


def measure_pairs(geo, seed=200):
    """350 + 440 and 480 + 620 Hz at -4, 0 and +4 dB twist, 300 frames each: (frames that are no pair, largest frequency error in Hz)"""
    rate, fft, shift, plan, t = setup(geo)
    rng = np.random.RandomState(seed)
    not_pair, worst = 0, 0.0
    for f1, f2 in ((350.0, 440.0), (480.0, 620.0)):
        for twist in (-4.0, 0.0, 4.0):
            frames = []
            for i in range(300):
                lev = rng.uniform(-24.0, -9.0)
                sig = R.sine(f1, fft, rate, lev, rng.uniform(0, 6.28)) + R.sine(f2, fft, rate, lev + twist, rng.uniform(0, 6.28))
                frames.append(R.to_pcm(sig + R.noise(fft, lev - 3.0 - 25.0, seed + len(frames) + int(f1))))
            rec, _ = A.tone_host(plan, t, np.stack(frames))
            ok = rec[:, 1] != 0
            not_pair += int((~ok).sum())
            if ok.any():
                worst = max(worst, float(np.abs(rec[ok, 0] - f1).max()), float(np.abs(rec[ok, 1] - f2).max()))
    return not_pair, worst


def measure_nontonal(geo="16k", count=2000):
    """tonal frames in `count` frames of white noise at -20 dBFS and in `count` frames of the harmonic voice-like signal"""
    rate, fft, shift, plan, t = setup(geo)
    n = (count - 1) * shift + fft
    out = []
    for pcm in (R.to_pcm(R.noise(n, -20.0, 300)), R.to_pcm(R.voice_like(n, rate, 301))):
        rec, pw = A.tone_host(plan, t, R.frames_of(pcm, fft, shift))
        assert len(rec) == count
        F = plan.F
        best = 0.0
        for q in pw:
            c = int(np.argmax(q[:F]))
            best = max(best, float(q[max(0, c - 1):c + 2].astype(np.float64).sum()) / max(1.0, float(q[F]) * float(plan.half_w)))
        out.append((int((rec[:, 0] != 0).sum()), best))
    return out


# measured with the seeds above (run this file as a script): the largest error of a single tone 3.52 Hz at W = 512, 4.58 Hz at W = 256,
# 5.30 Hz at W = 384, 1.92 Hz at W = 2048, smallest share 0.813; of a pair's component 12.0 Hz.  Asserted with a quarter on top (not less
# than 1 Hz)
SINGLE_ERR_HZ = {"16k": 3.52, "8k": 4.58, "n400": 5.30, "48k": 1.92}
PAIR_ERR_HZ = {"16k": 12.0, "8k": 12.0}


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_single_tones_are_found_with_their_frequency(built, geo):
    err, share, pairs, missed = measure_singles(geo)
    assert missed == 0 and pairs == 0, (missed, pairs)
    assert err <= SINGLE_ERR_HZ[geo] + max(1.0, 0.25 * SINGLE_ERR_HZ[geo]), err
    assert share >= 0.8, share                                                     # (measured: 0.813)


@pytest.mark.parametrize("geo", ["16k", "8k"])
def test_pairs_are_found_in_every_frame(built, geo):
    not_pair, worst = measure_pairs(geo)
    assert not_pair == 0
    assert worst <= PAIR_ERR_HZ[geo] + max(1.0, 0.25 * PAIR_ERR_HZ[geo]), worst


def test_noise_and_voice_give_no_tonal_frame(built):
    (noise_tonal, _), (voice_tonal, _) = measure_nontonal()
    assert noise_tonal == 0 and voice_tonal == 0


# ------------------------------------------------------------------ events
LEADS = (0, 53, 107, 159)                             # sub-frame alignments of the scenario
# measured on the numpy statement over LEADS (ms): ON time - true onset, OFF time - true end
ON_BOUNDS = (-24, -9)
OFF_BOUNDS = (-7, 1)


def scenario_events(lead, flush_ms=None):
    rate, fft, shift, plan, t = setup("16k")
    pcm, edges = R.sequence(R.SCENARIO, rate, -55.0, seed=5)
    pcm = np.concatenate([np.zeros(lead, np.int16), pcm])
    rec, _ = A.tone_host(plan, t, R.frames_of(pcm, fft, shift))
    ev, m = A.tone_events_host(plan, 10, 0, rec[:len(rec) // 3])
    ev2, m = A.tone_events_host(plan, 10, len(rec) // 3, rec[len(rec) // 3:], m, flush=True)
    want = R.events(plan_dict(plan), 10, 0, rec, R.machine())
    return tup(ev + ev2), want, [(a + lead / 16.0, b + lead / 16.0) for a, b in edges]


def scenario_deltas():
    on, off = [], []
    for lead in LEADS:
        ev, _, edges = scenario_events(lead)
        for (a, b), e_on, e_off in zip(edges, ev[0::2], ev[1::2]):
            on.append(e_on[3] - a); off.append(e_off[3] - b)
    return (min(on), max(on)), (min(off), max(off))


def test_scenario_gives_the_expected_events_with_their_names_and_times(built):
    for lead in LEADS:
        ev, want, edges = scenario_events(lead)
        assert ev == want, lead                                                    # the library's machine is the statement's
        assert [e[0] for e in ev] == [R.ON, R.OFF] * 4, (lead, ev)
        assert [A.tone_name(e[1], e[2]) for e in ev[0::2]] == R.SCENARIO_NAMES == [R.name(e[1], e[2]) for e in ev[0::2]], (lead, ev)
        assert all(on[1:3] == off[1:3] for on, off in zip(ev[0::2], ev[1::2]))     # OFF carries what its ON carried
        for (a, b), e_on, e_off in zip(edges, ev[0::2], ev[1::2]):
            assert ON_BOUNDS[0] <= e_on[3] - a <= ON_BOUNDS[1], (lead, a, e_on)
            assert OFF_BOUNDS[0] <= e_off[3] - b <= OFF_BOUNDS[1], (lead, b, e_off)
    on, off = scenario_deltas()
    assert (int(np.floor(on[0])), int(np.ceil(on[1]))) == ON_BOUNDS and (int(np.floor(off[0])), int(np.ceil(off[1]))) == OFF_BOUNDS, (on, off)


def test_frequency_step_and_flush_inside_a_tone(built):
    rate, fft, shift, plan, t = setup("16k")
    n = rate * 300 // 1000
    ph = 2 * np.pi * np.cumsum(np.concatenate([np.full(n, 1000.0), np.full(n, 1050.0)])) / rate      # (continuous phase: no click)
    pcm = R.to_pcm(0.25 * np.sin(ph) + R.noise(2 * n, -55.0, 8))
    rec, _ = A.tone_host(plan, t, R.frames_of(pcm, fft, shift))
    ev, _ = A.tone_events_host(plan, 10, 0, rec, flush=True)
    ev = tup(ev)
    assert [e[0] for e in ev] == [R.ON, R.OFF, R.ON, R.OFF], ev
    assert abs(ev[0][1] - 1000) <= 5 and abs(ev[2][1] - 1050) <= 5 and all(e[2] == 0 for e in ev), ev
    assert ev[1][1:3] == ev[0][1:3] and ev[3][1:3] == ev[2][1:3]
    assert 270 <= ev[1][3] <= 310 and ev[1][3] <= ev[2][3] <= 330, ev              # OFF, then ON from the frame that ended the hold
    assert ev[3][3] == len(rec) * 10                                               # the flush closes the held tone at frames_seen
    assert ev == R.events(plan_dict(plan), 10, 0, rec, R.machine()) + [(R.OFF, ev[2][1], 0, len(rec) * 10)]


def test_event_machine_on_hand_written_records(built):
    p63 = A.tone_plan(16000, 512, 10)                                       # on 6, off 3
    p11 = A.tone_plan(16000, 512, 10, dict(min_tone_ms=10, min_pause_ms=10))
    p22 = A.tone_plan(16000, 512, 10, dict(min_tone_ms=20, min_pause_ms=20, tol_hz=5))
    N, F = R.ON, R.OFF
    a, b, pr = (1100, 0), (1150, 0), (480, 620)
    z = (0, 0)
    cases = [
        (p63, [a] * 5 + [z] + [a] * 6 + [z] * 3, False, [(N, 1100, 0, 60), (F, 1100, 0, 120)]),      # a run one frame short gives nothing
        (p63, [a] * 5 + [b] * 6, True, [(N, 1150, 0, 50), (F, 1150, 0, 110)]),                       # a non-matching tonal frame restarts the run
        (p22, [a, a, a, b, b, b], True, [(N, 1100, 0, 0), (F, 1100, 0, 30), (N, 1150, 0, 40), (F, 1150, 0, 60)]),
        (p22, [a, a, z, a, z, a, z, z, z], False, [(N, 1100, 0, 0), (F, 1100, 0, 60)]),              # a matching frame restarts the pause count
        # the ON carries the frame that completed the run, which becomes the reference: 1108 still matches it, 1110 does not
        (p22, [(1100, 0), (1104, 0), (1108, 0), (1112, 0)], True, [(N, 1104, 0, 0), (F, 1104, 0, 40)]),
        (p22, [(1100, 0), (1104, 0), (1110, 0), (1112, 0), (1112, 0)], True, [(N, 1104, 0, 0), (F, 1104, 0, 20), (N, 1112, 0, 30), (F, 1112, 0, 50)]),
        (p11, [a, pr, (480, 0), z, pr], True, [(N, 1100, 0, 0), (F, 1100, 0, 10), (N, 480, 620, 10), (F, 480, 620, 20), (N, 480, 0, 20), (F, 480, 0, 30),
                                              (N, 480, 620, 40), (F, 480, 620, 50)]),
        (p63, [], True, []),
        (p63, [z, z, a], True, []),                                         # a flush discards a candidate
    ]
    for i, (plan, recs, fl, want) in enumerate(cases):
        r = np.array(recs, np.uint16).reshape(-1, 2)
        ev, m = A.tone_events_host(plan, 10, 0, r, flush=fl)
        assert tup(ev) == want, (i, tup(ev))
        rm = R.machine()
        ref = R.events(plan_dict(plan), 10, 0, r, rm) + (R.flush(10, len(r), rm) if fl else [])
        assert ref == want, (i, ref)
        for cut in range(len(r) + 1):                                       # any cut of the records gives the same events
            e1, mm = A.tone_events_host(plan, 10, 0, r[:cut])
            e2, mm = A.tone_events_host(plan, 10, cut, r[cut:], mm, flush=fl)
            assert tup(e1 + e2) == want, (i, cut)
    ev, _ = A.tone_events_host(p22, 10, 1000, np.array([a, a, z, z], np.uint16))
    assert tup(ev) == [(N, 1100, 0, 10000), (F, 1100, 0, 10020)]


def test_names(built):
    for name, f1, f2 in R.NAMES:
        assert A.tone_name(f1, f2) == name == R.name(f1, f2)
        assert A.tone_name(f1 + 20, f2 + 20 if f2 else 0) == name and A.tone_name(f1 + 21, f2) != name
    assert A.tone_name(350) is None and A.tone_name(440, 480) is None and A.tone_name(1000) is None
    assert A.tone_name(430, 0, 5) == "cp425" and A.tone_name(431, 0, 5) is None and A.tone_name(70000, 0, 200) is None


def test_refusals(built):
    L = _ffi.lib()
    out = _ffi.AprilxTonePlan()

    def plan(rate=16000, fft=512, shift=10, size=None, flags=0, **kw):
        d = dict(R.DEFAULTS); d.update(kw)
        o = _ffi.AprilxToneOptions(C.sizeof(_ffi.AprilxToneOptions) if size is None else size, d["min_level_dbfs"], d["second_db"], d["min_share"],
                                   d["tol_hz"], d["min_tone_ms"], d["min_pause_ms"], flags)
        rc = int(L.aprilx_tone_plan(rate, fft, shift, C.byref(o), C.byref(out)))
        assert (rc == 0) == (R.make_plan(rate, fft, shift, d) is not None and size is None and flags == 0), (rate, fft, kw)
        return rc
    assert plan() == 0
    nan = float("nan")
    bad = [dict(size=8), dict(flags=1), dict(min_level_dbfs=-70.5), dict(min_level_dbfs=0.5), dict(min_level_dbfs=nan), dict(second_db=2.9),
           dict(second_db=30.5), dict(second_db=nan), dict(min_share=0.0), dict(min_share=1.01), dict(min_share=nan), dict(tol_hz=0), dict(tol_hz=201),
           dict(min_tone_ms=9), dict(min_tone_ms=5001), dict(min_pause_ms=9), dict(min_pause_ms=5001), dict(shift=0),
           # the refused models: W / rate below 20 ms, a rate below 6000, W above 4096, fewer than 8 bins, more than 128 bins
           dict(rate=16000, fft=319), dict(rate=5999, fft=256), dict(rate=200000, fft=8192), dict(rate=16000, fft=4096), dict(rate=6000, fft=512),
           dict(rate=16000, fft=0)]
    assert [plan(**b) for b in bad] == [-1] * len(bad)
    edge = [dict(min_level_dbfs=-70.0), dict(min_level_dbfs=0.0), dict(second_db=3.0), dict(second_db=30.0), dict(min_share=1.0), dict(tol_hz=1),
            dict(tol_hz=200), dict(min_tone_ms=10, min_pause_ms=5000), dict(min_tone_ms=5000, min_pause_ms=10), dict(rate=16000, fft=320),
            dict(rate=6000, fft=256), dict(rate=96000, fft=4096), dict(rate=48000, fft=2048)]
    assert [plan(**e) for e in edge] == [0] * len(edge)
    assert R.grid(96000, 4096) == (4096, 13, 86)
    assert L.aprilx_tone_plan(16000, 512, 10, None, C.byref(out)) == -1
    buf = np.zeros(2 * 64 * 512, np.float32)
    assert L.aprilx_tone_tables(16000, 512, buf.ctypes.data, buf.size - 1) == -1
    assert L.aprilx_tone_tables(16000, 319, buf.ctypes.data, buf.size) == -1
    assert L.aprilx_tone_tables(16000, 512, None, buf.size) == -1
    assert L.aprilx_tone_tables(16000, 512, buf.ctypes.data, buf.size) == buf.size
    good = A.tone_plan(16000, 512, 10)
    fr = np.zeros((2, 512), np.int16); rec = np.zeros((2, 2), np.uint16)
    assert L.aprilx_tone_host(C.byref(good), buf.ctypes.data, 2, fr.ctypes.data, 511, rec.ctypes.data, None) == -1        # a stride below W
    assert L.aprilx_tone_host(C.byref(good), None, 2, fr.ctypes.data, 512, rec.ctypes.data, None) == -1
    assert L.aprilx_tone_host(C.byref(good), buf.ctypes.data, 2, fr.ctypes.data, 512, rec.ctypes.data, None) == 0
    assert L.aprilx_tone_decide_host(None, buf.ctypes.data) == -1
    broken = A.tone_plan(16000, 512, 10); broken.F = 129
    assert L.aprilx_tone_decide_host(C.byref(broken), buf.ctypes.data) == -1
    with pytest.raises(ValueError):
        A.tone_plan(16000, 512, 10, dict(second=1.0))


def _build_and_run(tmp_path, name, extra=()):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", *extra, "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", name + ".cc"), "-o", exe], timeout=600)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0 and "all checks passed" in out, out[-3000:]


def test_header_alone_under_sanitizers(built, tmp_path):
    _build_and_run(tmp_path, "tone_test", ["-ffp-contract=off"])


def test_staging_layout_with_the_sixth_array_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "staging_layout_tone_test")


if __name__ == "__main__":
    for g in sorted(GEOMETRIES):
        print("singles", g, measure_singles(g))
    for g in ("16k", "8k"):
        print("pairs", g, measure_pairs(g))
    print("nontonal (tonal frames, largest share): noise, voice", measure_nontonal())
    print("scenario ON / OFF deltas (ms)", scenario_deltas())
