"""Voice activity without a GPU: the contract in plain C++ (aprilx_vad_host, aprilx_vad_plan_tables,
aprilx_vad_events_host; csrc/vad.h) against its numpy statement (tests/vad_ref.py) on every bit, the hand-derived cases
(tests/golden/vad_cases.py) against both, every refusal of the option ranges, and the header alone under AddressSanitizer + UBSan
as a stand-alone program (tests/cpp/vad_test.cc)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import april_asr_amd as A
from april_asr_amd import _ffi
import vad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import vad_cases as G  # noqa: E402

CSRC = os.path.join(ROOT, "april_asr_amd", "csrc")
NBINS = 80
NB_SET = (1, 15, 16, 17, 54, 80)


def c_plan(p):
    return _ffi.AprilxVadPlan(p["b0"], p["b1"], float(p["inv_nb"]), float(p["thr_on"]), float(p["thr_off"]), float(p["min_energy"]),
                              p["onset_frames"], p["hangover_frames"])


def c_state_tuple(st):
    fl = np.array([st.s, st.cur] + list(st.hist), np.float32).view(np.uint32).tolist()
    return tuple(fl) + (st.cnt, st.pos, st.st, st.run, st.first)


def band_plan(nb, rng, **kw):
    b0 = int(rng.randint(0, NBINS - nb + 1))
    d = dict(b0=b0, b1=b0 + nb, inv_nb=R.F(1.0) / R.F(nb), thr_on=R.F(5.0) * R.DB, thr_off=R.F(3.0) * R.DB, min_energy=R.F(-12.0),
             onset_frames=5, hangover_frames=30)
    d.update(kw)
    return d


def random_rows(rng, n):
    """log-mel-like rows with quiet and loud stretches, so that the state machine moves; some pad-value rows, -0.0 and large values"""
    level = np.repeat(rng.choice([-14.0, -9.0, -5.0, 0.0], size=(n + 19) // 20), 20)[:n]
    x = (level[:, None] + rng.normal(0, 1.5, size=(n, NBINS))).astype(np.float32)
    x[rng.rand(n) < 0.05] = np.float32(np.log(np.float64(1.1920928955078125e-07)))
    x[rng.rand(n, NBINS) < 0.01] = np.float32(-0.0)
    return x


@pytest.mark.parametrize("nb", NB_SET)
def test_host_equals_numpy_on_every_bit(built, nb):
    rng = np.random.RandomState(100 + nb)
    lengths = sorted(set([1, 2, 15, 16, 17, 31, 32, 33, 255, 256, 257, 288, 289, 400] + rng.randint(1, 401, size=6).tolist()))
    moved = 0
    for n in lengths:
        plan = band_plan(nb, rng)
        rows = random_rows(rng, n)
        want_b, want_e, want_v = R.run(plan, rows)
        got_b, got_e, got_v = A.vad_host(c_plan(plan), rows)
        assert (got_b == want_b).all(), (nb, n)
        assert (got_e.view(np.uint32) == want_e.view(np.uint32)).all(), (nb, n)
        assert c_state_tuple(got_v) == R.state_tuple(want_v), (nb, n)
        moved += int((want_b & 1).any() and not (want_b & 1).all())
    assert moved >= 3                      # the inputs do exercise both states


def test_cut_sequence_equals_the_uncut_run(built):
    rng = np.random.RandomState(7)
    for nb in NB_SET:
        plan = band_plan(nb, rng)
        rows = random_rows(rng, 400)
        whole_b, whole_e, whole_v = A.vad_host(c_plan(plan), rows)
        cuts = sorted(set(rng.randint(1, 400, size=9).tolist() + [1, 32, 33]))
        st, ref_v, bs, rbs = A.vad_reset_state(), None, [], []
        for a, b in zip([0] + cuts, cuts + [400]):
            pb, _, st = A.vad_host(c_plan(plan), rows[a:b], st)
            rb, _, ref_v = R.run(plan, rows[a:b], ref_v)
            bs.append(pb); rbs.append(rb)
        assert (np.concatenate(bs) == whole_b).all() and (np.concatenate(rbs) == whole_b).all()
        assert c_state_tuple(st) == c_state_tuple(whole_v) == R.state_tuple(ref_v)


@pytest.mark.parametrize("case", G.CASES, ids=[c["name"] for c in G.CASES])
def test_hand_derived_cases(built, case):
    rows = np.array(case["e"], np.float32).reshape(-1, 1)
    want = np.array(case["want"], np.uint8)
    ref_b, ref_e, _ = R.run(case["plan"], rows)
    assert (ref_e == rows[:, 0]).all()                      # one bin, inv_nb 1: the energy is the row's value
    assert ref_b.tolist() == want.tolist()
    got_b, got_e, _ = A.vad_host(c_plan(case["plan"]), rows)
    assert got_b.tolist() == want.tolist() and (got_e == rows[:, 0]).all()
    # the case tells its comparison from the changed one
    mut_b, _, _ = R.run(case["plan"], rows, mut=case["mutant"])
    assert mut_b.tolist() != want.tolist(), case["mutant"]


def test_open_segment_is_closed_by_the_flush(built):
    case = [c for c in G.CASES if c["name"] == "open_segment_at_flush"][0]
    ev, last = A.vad_events_host(c_plan(case["plan"]), 10, 0, case["want"], 0)
    assert [(e.kind, e.time_ms) for e in ev] == [(R.START, 10)] and last == 1
    assert R.flush_end(len(case["want"]), 10, last) == [(R.END, 40)]


@pytest.mark.parametrize("case", G.EVENT_CASES)
def test_event_times_follow_from_the_bytes(built, case):
    plan = G.plan(onset=case["onset"], hang=case["hang"])
    want = case["want"]
    ref, ref_last = R.events(plan, case["shift"], case["t0"], case["data"], 0)
    got, last = A.vad_events_host(c_plan(plan), case["shift"], case["t0"], case["data"], 0)
    assert ref == want and [(e.kind, e.time_ms) for e in got] == want
    assert ref_last == last == case["last"]
    assert R.flush_end(case["t0"] + len(case["data"]), case["shift"], last) == case["open_end"]
    # cut anywhere, carried through the last bit: the same events
    for k in range(len(case["data"]) + 1):
        a, l1 = A.vad_events_host(c_plan(plan), case["shift"], case["t0"], case["data"][:k], 0)
        b, l2 = A.vad_events_host(c_plan(plan), case["shift"], case["t0"] + k, case["data"][k:], l1)
        assert [(e.kind, e.time_ms) for e in a + b] == want and l2 == last


def test_events_of_random_bytes(built):
    rng = np.random.RandomState(3)
    plan = G.plan(onset=3, hang=7)
    data = (np.repeat(rng.randint(0, 2, size=40), rng.randint(1, 9, size=40)) | (rng.randint(0, 2, size=1)[0] << 1)).astype(np.uint8)
    ref, ref_last = R.events(plan, 10, 6, data, 0)
    got, last = A.vad_events_host(c_plan(plan), 10, 6, data, 0)
    assert [(e.kind, e.time_ms) for e in got] == ref and last == ref_last and len(ref) >= 8


def synthetic_mel(nbins=8, nfft=64):
    """triangles with peaks at fft bins 4, 8, ..., the last row with a flat top (two equal maxima: the first counts)"""
    mel = np.zeros((nbins, nfft), np.float32)
    for b in range(nbins):
        c = 4 * (b + 1)
        for k in range(c - 3, c + 4):
            mel[b, k] = 1.0 - abs(k - c) / 4.0
    mel[nbins - 1, 4 * nbins + 1] = 1.0
    return mel


def test_band_derives_from_a_mel_table(built):
    mel = synthetic_mel()
    rate, shift = 6400, 10                                  # fft bin k is k * 50 Hz: the peaks are at 200, 400, ..., 1600 Hz
    for lo, hi, want in ((200.0, 1600.0, (0, 8)), (201.0, 1599.0, (1, 7)), (0.0, 3200.0, (0, 8)), (400.0, 400.0001, (1, 2)), (1600.0, 1650.0, (7, 8))):
        o = R.options(band_lo_hz=lo, band_hi_hz=hi, onset_ms=55, hangover_ms=19)
        ref = R.make_plan(mel, rate, shift, o)
        got = A.vad_plan(mel, rate, shift, o)
        assert (ref["b0"], ref["b1"]) == want == (got.b0, got.b1), (lo, hi)
        assert (got.onset_frames, got.hangover_frames) == (5, 1) == (ref["onset_frames"], ref["hangover_frames"])
        for f in ("inv_nb", "thr_on", "thr_off", "min_energy"):
            assert np.float32(getattr(got, f)).view(np.uint32) == np.float32(ref[f]).view(np.uint32), f
    # a band that holds no peak is refused
    for lo, hi in ((210.0, 390.0), (1700.0, 3200.0), (0.0, 150.0)):
        assert R.make_plan(mel, rate, shift, R.options(band_lo_hz=lo, band_hi_hz=hi)) is None
        with pytest.raises(ValueError):
            A.vad_plan(mel, rate, shift, dict(band_lo_hz=lo, band_hi_hz=hi))


def test_the_tiny_models_band(built, tiny_model):
    m = A.Model.load_host_only(tiny_model["path"])
    _, mel = m.fbank_tables()
    d = m.dims
    shift_ms = d.frame_shift * 1000 // d.sample_rate
    ref = R.make_plan(mel, d.sample_rate, shift_ms, R.options())
    got = A.vad_plan(mel, d.sample_rate, shift_ms, True)
    assert (got.b0, got.b1) == (ref["b0"], ref["b1"]) and got.b1 - got.b0 >= 1
    assert (got.onset_frames, got.hangover_frames) == (50 // shift_ms, 300 // shift_ms)
    assert np.float32(got.thr_on) == np.float32(5.0) * R.DB and np.float32(got.thr_off) == np.float32(3.0) * R.DB


def test_every_refusal_of_the_option_ranges(built):
    mel = synthetic_mel()
    L = _ffi.lib()
    plan = _ffi.AprilxVadPlan()

    def call(size=None, flags=0, **kw):
        d = dict(A._VAD_DEFAULTS, band_lo_hz=200.0, band_hi_hz=1600.0)
        d.update(kw)
        o = _ffi.AprilxVadOptions(C.sizeof(_ffi.AprilxVadOptions) if size is None else size, d["band_lo_hz"], d["band_hi_hz"], d["onset_db"],
                                  d["offset_db"], d["onset_ms"], d["hangover_ms"], d["min_energy"], flags)
        rc = int(L.aprilx_vad_plan_tables(mel.ctypes.data, mel.shape[0], mel.shape[1], 6400, 10, C.byref(o), C.byref(plan)))
        if size is None and flags == 0:
            assert (rc == 0) == (R.make_plan(mel, 6400, 10, d) is not None), kw
        return rc
    inf, nan = float("inf"), float("nan")
    assert call() == 0
    assert call(size=32) == -1 and call(size=0) == -1 and call(flags=1) == -1
    # the band: 0 <= lo < hi <= rate / 2
    assert call(band_lo_hz=-1.0) == -1 and call(band_lo_hz=1600.0) == -1 and call(band_lo_hz=1700.0) == -1
    assert call(band_hi_hz=3200.0) == 0 and call(band_hi_hz=3200.5) == -1
    assert call(band_lo_hz=nan) == -1 and call(band_hi_hz=nan) == -1 and call(band_hi_hz=inf) == -1
    assert call(band_lo_hz=0.0) == 0
    # thresholds: finite, 0 < offset <= onset <= 60
    assert call(offset_db=0.0) == -1 and call(offset_db=-1.0) == -1 and call(offset_db=5.0) == 0 and call(offset_db=5.5) == -1
    assert call(onset_db=60.0) == 0 and call(onset_db=60.5) == -1 and call(onset_db=nan) == -1 and call(offset_db=nan) == -1
    assert call(onset_db=inf) == -1
    # counts: 10 .. 1000 ms and 10 .. 10000 ms
    assert call(onset_ms=9) == -1 and call(onset_ms=10) == 0 and call(onset_ms=1000) == 0 and call(onset_ms=1001) == -1
    assert call(hangover_ms=9) == -1 and call(hangover_ms=10) == 0 and call(hangover_ms=10000) == 0 and call(hangover_ms=10001) == -1
    assert call(min_energy=nan) == -1 and call(min_energy=inf) == -1 and call(min_energy=-inf) == -1 and call(min_energy=3.0) == 0
    # bad arguments of the host entry points
    assert int(L.aprilx_vad_plan_tables(None, 8, 64, 6400, 10, C.byref(A._vad_options(True)), C.byref(plan))) == -1
    assert int(L.aprilx_vad_plan_tables(mel.ctypes.data, 8, 64, 6400, 10, None, C.byref(plan))) == -1
    st = A.vad_reset_state()
    rows = np.zeros((2, 4), np.float32); b = np.zeros(2, np.uint8)
    bad = _ffi.AprilxVadPlan(0, 5, 0.2, 1.0, 0.5, -12.0, 1, 1)                # the band reaches past the row
    assert int(L.aprilx_vad_host(C.byref(bad), 2, 4, rows.ctypes.data, C.byref(st), b.ctypes.data, None)) == -1
    ok = _ffi.AprilxVadPlan(0, 4, 0.25, 1.0, 0.5, -12.0, 1, 1)
    assert int(L.aprilx_vad_host(C.byref(ok), 2, 4, rows.ctypes.data, C.byref(st), b.ctypes.data, None)) == 0
    assert int(L.aprilx_vad_host(C.byref(ok), 2, 4, rows.ctypes.data, None, b.ctypes.data, None)) == -1
    with pytest.raises(ValueError):
        A._vad_options(dict(onset=3))


def test_header_alone_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "vad_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "vad_test.cc"), "-o", exe], timeout=600)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0 and "all checks passed" in out, out[-3000:]
