"""DTMF without a GPU: the contract in plain C++ (aprilx_dtmf_plan, aprilx_dtmf_tables, aprilx_dtmf_host,
aprilx_dtmf_decide_host, aprilx_dtmf_events_host; csrc/dtmf.h) against its numpy statement (tests/dtmf_ref.py) on every bit, decoded
digit strings with their times, the twist / level limits, exact ties, every refusal, the event machine on hand-written codes, and the
header alone under AddressSanitizer + UBSan as a stand-alone program (tests/cpp/dtmf_test.cc)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import april_asr_amd as A
from april_asr_amd import _ffi
from conftest import speech_like_pcm
import dtmf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "april_asr_amd", "csrc")
# (rate, fft_size, frame shift in samples): 16 kHz / 25 ms (Wd 256), 8 kHz (Wd 128), 12.5 ms without rounding up (Wd 200: a ragged last
# chain), and 13 ms (Wd 208), the nearest a model file -- whole milliseconds -- comes to it
# ... and 48 kHz (Wd 768: twelve links per chain)
GEOMETRIES = {"16k": (16000, 512, 160), "8k": (8000, 256, 80), "n200": (16000, 200, 160), "n208": (16000, 208, 160), "48k": (48000, 2048, 480)}


def plan_dict(p):
    return dict(Wd=p.Wd, half_w=R.F(p.half_w), min_power=R.F(p.min_power), twist_hi=R.F(p.twist_hi), twist_lo=R.F(p.twist_lo), rel_peak=R.F(p.rel_peak),
                min_share=R.F(p.min_share), on_frames=p.on_frames, off_frames=p.off_frames)


def setup(geo, options=True):
    rate, fft, shift = GEOMETRIES[geo]
    plan = A.dtmf_plan(rate, fft, 10, options)
    return rate, fft, shift, plan, A.dtmf_tables(rate, plan.Wd)


def same_bits(a, b):
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def decode(plan, codes, flush_at=None):
    """the library's events of a whole code string (fed in two uneven parts: the machine carries over)"""
    k = len(codes) // 3
    ev1, m = A.dtmf_events_host(plan, 10, 0, codes[:k])
    ev2, m = A.dtmf_events_host(plan, 10, k, codes[k:], m, flush=flush_at is not None)
    return [(e.kind, e.digit, e.time_ms) for e in ev1 + ev2]


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_tables_and_plan(built, geo):
    rate, fft, shift, plan, t = setup(geo)
    assert plan.Wd == R.window(rate, fft) == {"16k": 256, "8k": 128, "n200": 200, "n208": 208, "48k": 768}[geo]
    assert np.abs(t.astype(np.float64) - R.tables_f64(rate, plan.Wd)).max() <= 1e-7
    want = R.make_plan(rate, fft, 10, R.options())
    got = plan_dict(plan)
    for k in ("Wd", "on_frames", "off_frames", "half_w", "min_share"):
        assert got[k] == want[k], k
    for k in ("min_power", "twist_hi", "twist_lo", "rel_peak"):                   # (pow() of two libms: within an ulp of fp32)
        assert abs(float(got[k]) - float(want[k])) <= 1.2e-7 * float(want[k]), k
    assert (got["on_frames"], got["off_frames"]) == (2, 2)


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_host_equals_numpy_on_every_bit_and_decodes_the_string(built, geo):
    rate, fft, shift, plan, t = setup(geo)
    p = plan_dict(plan)
    seen = 0
    for tone_ms, pause_ms in ((40, 40), (45, 45)):
        for noise in (-50.0, -30.0):
            for lead in (0, shift // 3, shift - 1):                                # three sub-frame alignments
                pcm, onsets = R.digit_signal(R.STRING, tone_ms, pause_ms, rate, noise, lead, seed=lead + tone_ms)
                frames = R.frames_of(pcm, fft, shift)
                codes, pw = A.dtmf_host(plan, t, frames)
                want_c, want_p = R.run(p, t, frames)
                assert codes.tolist() == want_c.tolist(), (geo, tone_ms, noise, lead)
                assert same_bits(pw, want_p), (geo, tone_ms, noise, lead)
                ev = decode(plan, codes)
                assert ev == R.events(p, 10, 0, codes, R.machine())
                seen += int((codes != 0).sum())
                if geo not in ("16k", "8k"):               # (the other windows -- 12.5 ms resolves 80 Hz, the rows lie 73 Hz apart --: bits only)
                    continue
                assert R.digits_of(ev) == R.STRING, (geo, tone_ms, noise, lead, R.digits_of(ev))
                downs = [tm for k, _, tm in ev if k == R.DOWN]
                ups = [tm for k, _, tm in ev if k == R.UP]
                assert len(ups) == len(downs) == len(R.STRING) == 26
                # DOWN is the start of the first of on_frames detecting frames: a frame that starts more than a window before the onset
                # holds no tone, and the first frame that starts at or behind the onset -- less than one shift later -- and its
                # successor lie inside the tone (16 + 10 + 10 ms < 40 ms)
                for on_s, dn, up in zip(onsets, downs, ups):
                    on_ms = on_s * 1000.0 / rate
                    assert -16.0 < dn - on_ms < 10.0, (geo, on_ms, dn)
                    assert dn + 20 <= up <= on_ms + tone_ms + 10.0, (geo, on_ms, tone_ms, dn, up)
    assert seen > 26 * 12 * 2 or geo not in ("16k", "8k")


def test_edge_signals_equal_numpy(built):
    for geo in sorted(GEOMETRIES):
        rate, fft, shift, plan, t = setup(geo)
        p = plan_dict(plan)
        rng = np.random.RandomState(3)
        n = 40 * shift + fft
        square = np.where(np.sin(2 * np.pi * 697.0 * np.arange(n) / rate) >= 0, 32767, -32768).astype(np.int16)
        edges = rng.choice(np.array([-32768, 32767, -32767, 0, 1, -1], np.int16), size=n)
        lowest = np.full(n, -32768, np.int16)
        for name, pcm in (("silence", np.zeros(n, np.int16)), ("square", square), ("edges", edges), ("lowest", lowest)):
            frames = R.frames_of(pcm, fft, shift)
            codes, pw = A.dtmf_host(plan, t, frames)
            want_c, want_p = R.run(p, t, frames)
            assert codes.tolist() == want_c.tolist() and same_bits(pw, want_p), (geo, name)
            assert name == "square" or not codes.any(), (geo, name)                # no tone pair holds 0.6 of their energy
        assert float(pw[0, 8]) == float(plan.Wd) * 2.0 ** 30                        # the energy of Wd samples of -32768, exactly


def steady_codes(geo, options=True, **kw):
    rate, fft, shift, plan, t = setup(geo, options)
    pcm = np.clip(np.round(R.tone("5", rate // 2, rate, **kw) * 32768.0), -32768, 32767).astype(np.int16)
    codes, _ = A.dtmf_host(plan, t, R.frames_of(pcm, fft, shift))
    assert len(codes) > 40
    return codes


@pytest.mark.parametrize("geo", ["16k", "8k"])
def test_twist_and_level_limits(built, geo):
    five = 1 + R.DIGITS.index("5")
    for twist, ok in ((3.0, True), (5.0, False), (-7.0, True), (-9.0, False)):
        codes = steady_codes(geo, level_dbfs=-16.0 if twist > 0 else -12.0, twist_db=twist)
        assert (codes == (five if ok else 0)).all(), (twist, codes.tolist())
    assert not steady_codes(geo, level_dbfs=-48.0).any()
    assert (steady_codes(geo, level_dbfs=-34.0) == five).all()
    assert (steady_codes(geo, dict(min_level_dbfs=-50.0), level_dbfs=-48.0) == five).all()      # (the floor is what refused it)


def test_no_detection_on_speech_like_audio(built):
    rate, fft, shift, plan, t = setup("16k")
    for seed in range(3):
        codes, _ = A.dtmf_host(plan, t, R.frames_of(speech_like_pcm(3.0, seed=seed), fft, shift))
        assert len(codes) > 290 and not codes.any(), seed


def test_exact_ties_in_the_decision(built):
    for geo in ("16k", "8k"):
        _, _, _, plan, _ = setup(geo)
        p = plan_dict(plan)
        for i, (q, code) in enumerate(R.tie_rows(p)):
            assert R.decide(p, q) == code, (geo, i)
            assert A.dtmf_decide_host(plan, q) == code, (geo, i)


def test_refusals(built):
    L = _ffi.lib()
    out = _ffi.AprilxDtmfPlan()

    def plan(rate=16000, fft=512, shift=10, size=None, flags=0, **kw):
        d = dict(R.DEFAULTS); d.update(kw)
        o = _ffi.AprilxDtmfOptions(C.sizeof(_ffi.AprilxDtmfOptions) if size is None else size, d["min_level_dbfs"], d["twist_hi_db"], d["twist_lo_db"],
                                   d["rel_peak_db"], d["min_share"], d["min_tone_ms"], d["min_pause_ms"], flags)
        rc = int(L.aprilx_dtmf_plan(rate, fft, shift, C.byref(o), C.byref(out)))
        assert (rc == 0) == (R.make_plan(rate, fft, shift, d) is not None and size is None and flags == 0), (rate, fft, kw)
        return rc
    assert plan() == 0
    nan = float("nan")
    bad = [dict(size=8), dict(flags=1), dict(min_level_dbfs=-70.5), dict(min_level_dbfs=0.5), dict(min_level_dbfs=nan), dict(twist_hi_db=-0.1),
           dict(twist_hi_db=20.5), dict(twist_lo_db=-1.0), dict(twist_lo_db=21.0), dict(twist_lo_db=nan), dict(rel_peak_db=2.9), dict(rel_peak_db=30.5),
           dict(min_share=0.0), dict(min_share=1.01), dict(min_share=nan), dict(min_tone_ms=9), dict(min_tone_ms=1001), dict(min_pause_ms=9),
           dict(min_pause_ms=1001), dict(shift=0),
           dict(rate=3999, fft=128), dict(rate=16000, fft=191), dict(rate=4000, fft=47), dict(rate=7999, fft=256), dict(rate=300000, fft=8192)]
    assert [plan(**b) for b in bad] == [-1] * len(bad)
    edge = [dict(min_level_dbfs=-70.0), dict(min_level_dbfs=0.0), dict(twist_hi_db=0.0, twist_lo_db=20.0), dict(rel_peak_db=3.0), dict(rel_peak_db=30.0),
            dict(min_share=1.0), dict(min_tone_ms=10, min_pause_ms=1000), dict(rate=16000, fft=192), dict(rate=4000, fft=64), dict(rate=8000, fft=128), dict(rate=256000, fft=8192)]
    assert [plan(**e) for e in edge] == [0] * len(edge)
    assert L.aprilx_dtmf_plan(16000, 512, 10, None, C.byref(out)) == -1
    buf = np.zeros(16 * 256, np.float32)
    assert L.aprilx_dtmf_tables(16000, 256, buf.ctypes.data, buf.size - 1) == -1
    assert L.aprilx_dtmf_tables(16000, 0, buf.ctypes.data, buf.size) == -1
    assert L.aprilx_dtmf_tables(16000, 4097, buf.ctypes.data, 1 << 20) == -1
    assert L.aprilx_dtmf_tables(16000, 256, None, buf.size) == -1
    good = A.dtmf_plan(16000, 512, 10)
    fr = np.zeros((2, 512), np.int16); codes = np.zeros(2, np.uint8)
    assert L.aprilx_dtmf_host(C.byref(good), buf.ctypes.data, 2, fr.ctypes.data, 255, codes.ctypes.data, None) == -1        # a stride below Wd
    assert L.aprilx_dtmf_host(C.byref(good), None, 2, fr.ctypes.data, 512, codes.ctypes.data, None) == -1
    assert L.aprilx_dtmf_host(C.byref(good), buf.ctypes.data, 2, fr.ctypes.data, 512, codes.ctypes.data, None) == 0
    assert L.aprilx_dtmf_decide_host(None, buf.ctypes.data) == -1


def test_event_machine_on_hand_written_codes(built):
    p22 = A.dtmf_plan(16000, 512, 10)                                       # on = off = 2
    p11 = A.dtmf_plan(16000, 512, 10, dict(min_tone_ms=10, min_pause_ms=10))
    p32 = A.dtmf_plan(16000, 512, 10, dict(min_tone_ms=30))
    p23 = A.dtmf_plan(16000, 512, 10, dict(min_pause_ms=30))
    D, U = R.DOWN, R.UP
    cases = [
        # a run one frame short gives nothing; the next one counts from its own first frame
        (p22, [0, 5, 0, 0, 5, 5, 0, 0], False, [(D, "4", 40), (U, "4", 60)]),
        (p32, [9, 9, 0, 9, 9, 3, 9, 9, 9, 0, 0], False, [(D, "7", 60), (U, "7", 90)]),
        # a digit change without a pause: UP, then DOWN from the frame that ended the hold
        (p22, [1, 1, 1, 6, 6, 6], True, [(D, "1", 0), (U, "1", 30), (D, "5", 40), (U, "5", 60)]),
        # a flush inside a digit closes it at frames_seen
        (p22, [0, 2, 2, 2], True, [(D, "2", 10), (U, "2", 40)]),
        # a single frame of the held code restarts the pause count
        (p22, [1, 1, 0, 1, 0, 1, 0, 0, 0], False, [(D, "1", 0), (U, "1", 60)]),
        # on = off = 1: every change is an event at its own frame
        (p11, [3, 3, 4, 0, 16], True, [(D, "3", 0), (U, "3", 20), (D, "A", 20), (U, "A", 30), (D, "D", 40), (U, "D", 50)]),
        # ... a new code in every frame: two events per frame, 2 n in all with the flush's
        (p11, [1, 2, 3, 4, 5], True, [(D, "1", 0), (U, "1", 10), (D, "2", 10), (U, "2", 20), (D, "3", 20), (U, "3", 30), (D, "A", 30), (U, "A", 40),
                                      (D, "4", 40), (U, "4", 50)]),
        # a hold interrupted by ANOTHER key for off_frames - 1 frames goes on; off_frames of it end the hold, and the frame that ended it
        # counts as the other key's first
        (p23, [1, 1, 5, 5, 1, 5, 5, 5], True, [(D, "1", 0), (U, "1", 50)]),
        (p23, [1, 1, 5, 5, 1, 5, 5, 5, 5, 0, 0, 0], False, [(D, "1", 0), (U, "1", 50), (D, "4", 70), (U, "4", 90)]),
        # ... and while a key is held, a run of another key gives no DOWN of its own, however long the candidate would have been
        (p23, [2, 2, 6, 6, 2, 2, 6, 6, 2], True, [(D, "2", 0), (U, "2", 90)]),
        (p22, [], True, []),
        (p22, [0, 0, 9], True, []),                                         # a flush discards a candidate
    ]
    for i, (plan, codes, fl, want) in enumerate(cases):
        ev, m = A.dtmf_events_host(plan, 10, 0, np.array(codes, np.uint8), flush=fl)
        got = [(e.kind, e.digit, e.time_ms) for e in ev]
        assert got == want, (i, got)
        rm = R.machine()
        ref = R.events(plan_dict(plan), 10, 0, codes, rm) + (R.flush(10, len(codes), rm) if fl else [])
        assert ref == want, (i, ref)
        assert (m.held, m.cand, m.run) == (rm["held"], rm["cand"], rm["run"]), i
        # any cut of the code string gives the same events
        for cut in range(len(codes) + 1):
            e1, mm = A.dtmf_events_host(plan, 10, 0, np.array(codes[:cut], np.uint8))
            e2, mm = A.dtmf_events_host(plan, 10, cut, np.array(codes[cut:], np.uint8), mm, flush=fl)
            assert [(e.kind, e.digit, e.time_ms) for e in e1 + e2] == want, (i, cut)
    # a frame offset moves the times only
    ev, _ = A.dtmf_events_host(p22, 10, 1000, np.array([5, 5, 0, 0], np.uint8))
    assert [(e.kind, e.digit, e.time_ms) for e in ev] == [(D, "4", 10000), (U, "4", 10020)]


def test_header_alone_under_sanitizers(built, tmp_path):
    exe = str(tmp_path / "dtmf_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "dtmf_test.cc"), "-o", exe], timeout=600)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0 and "all checks passed" in out, out[-3000:]
