"""Line quality per session (aprilx_session_set_quality): quality_kernel against the numpy statement of the contract
(tests/quality_ref.py), every bit of the records; live sessions in every ingest mode, whose events must be the statement applied to the
session's own model-rate samples (PCM16 at 16 kHz, mu-law at 8 kHz through the resampler, channel 1 of two float32 channels), each
beside a twin without the observer that must not differ in anything; a session with all three detectors and the observer beside one with
the detectors only; an engine without an opted-in session, which must launch nothing; and the refusals that need a live session.
Every scenario runs in a child process (tests/quality_worker.py)."""
import json
import os
import subprocess
import sys

import pytest

import quality_ref as R
from quality_worker import LEVELS, N_SET

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(path, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "quality_worker.py"), path] + [str(a) for a in args],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.fixture(scope="module")
def models(model_dir, tiny_model):
    """the tiny model (16 kHz: H 160, two and a half slabs of 64), the same at 8 kHz (H 80) and at 48 kHz (H 480)"""
    from april_asr_amd import synth_model as SM
    out = {"16k": (tiny_model["path"], 160)}
    for name, params, hop in (("8k", dict(rate=8000), 80), ("48k", dict(rate=48000), 480)):
        p = str(model_dir / ("quality_%s.april" % name))
        SM.write_model(p, SM.TINY_DIMS, params=params)
        out[name] = (p, hop)
    return out


@pytest.mark.parametrize("geo", ["16k", "8k", "48k"])
def test_kernel_equals_the_contract_bitwise(built, models, geo):
    """aprilx_run_quality: runs of 1, 3, 4, 5 and 257 frames at three clip levels, the whole pool of special frames (the CPU test's
    inputs and clip runs, the extreme sample in lane 63 and at H - 1), three runs with different clip levels in one launch"""
    path, hop = models[geo]
    r = run(path, "kernel")
    assert r["hop"] == hop
    assert r["calls"] == len(N_SET) * len(LEVELS) + 2
    assert r["host_bad"] == [] and r["bad"] == [], r["bad"][:10]
    assert r["clipped"] >= 10 and r["dead"] >= 6, r                   # (the frames do hold clipping and dead frames)
    assert r["differ"] == 2, r["differ"]                              # ... and the clip level of a run does change what comes out
    assert r["refusals"] == [-1, -1, -1, -1, -1, 0], r["refusals"]


@pytest.mark.parametrize("mode", ["sync", "async", "pipe2"])
def test_live_sessions_equal_the_contract_on_their_own_samples(built, tiny_model, mode):
    """2.6 s with an overdriven stretch, digital silence (a flush falls into it) and a stuck value: two PCM16 streams with different
    options, a mu-law stream at 8000 Hz and a two-channel float32 stream taking channel 1, EACH beside a twin without the observer (same
    format, same bytes, same group) whose token events, feature rows and chunk count must be the same: 100 ms feeds and irregular feeds"""
    chunkings = ["100ms", "irregular"]
    res = run(tiny_model["path"], "live", mode, *chunkings)
    for c in chunkings:
        r = res[c]
        assert r["mismatch"] == 0, c
        assert len(r["streams"]) == 4
        for s in r["streams"]:
            assert s["cku"] == 0 and s["hop"] == 160, (c, s)
            assert s["host_equal"] and s["equal"], (c, s["got"], s["want"])
            assert s["frames_seen"] == s["real"] and s["counters"] == s["want_counters"] and s["state"] == [0, 0], (c, s)
        first, second, tel, two = r["streams"]
        assert first["n_want"] >= 30 and first["kinds"] == [1, 2, 3, 4, 5], (c, first["kinds"])
        # the flush completes inside the hold of the overdriven stretch and inside the silence: both are closed at the segment's last frame
        assert first["closing"] == [R.CLIPPING_OFF, R.DROPOUT_OFF], (c, first["closing"])
        assert second["kinds"] == [1, 2, 3, 4, 5] and second["want_counters"][3] > first["want_counters"][3] > 0 < first["want_counters"][1], (c, second)      # (more samples reach the lower level)
        assert tel["n_want"] >= 15 and R.DROPOUT_ON in tel["kinds"] and tel["want_counters"][2] > 0, (c, tel)
        assert R.REPORT not in two["kinds"] and two["want_counters"][4] == 0 and {2, 3, 4, 5} <= set(two["kinds"]), (c, two)      # report_ms 0
        assert len(r["twins"]) == 4
        for t in r["twins"]:
            assert t["events"] and t["frames"] and t["chunks"], (c, t)
            assert t["n_events"] >= 1 and t["n_chunks"] >= 5 and t["twin_quality"] == 0 and t["twin_info"], (c, t)
        assert r["launches"] > 0 and r["quality_frames"] == r["want_quality_frames"], (c, r["quality_frames"], r["want_quality_frames"])


def test_all_detectors_and_the_observer_in_the_same_passes(built, tiny_model):
    """four sessions of one group on the same 2 s (irregular feeds, a flush in the middle): the three detectors and the observer, the
    detectors only, the observer only, nothing.  The passes carry descriptors of all four kinds, so their quality records sit behind the
    VAD and DTMF bytes and the tone records; each detector's events are those of the run without the observer, the observer's those of
    the numpy statement, and nobody's transcript may move"""
    r = run(tiny_model["path"], "all4")
    all4, det_only, q_only, neither = range(4)
    assert r["mismatch"] == 0 and r["single_frame_feeds"] >= 1, r["single_frame_feeds"]
    assert len(r["vad"][det_only]) >= 2 and r["vad"][all4] == r["vad"][det_only], (r["vad"][all4], r["vad"][det_only])
    assert len(r["keys"][det_only]) >= 4 and r["keys"][all4] == r["keys"][det_only], (r["keys"][all4], r["keys"][det_only])
    assert len(r["tones"][det_only]) >= 6 and r["tones"][all4] == r["tones"][det_only], (r["tones"][all4], r["tones"][det_only])
    assert len(r["want_quality"]) >= 10 and r["kinds"] == [1, 2, 3, 4, 5], r["kinds"]
    assert r["quality"][all4] == r["quality"][q_only] == r["want_quality"], (r["quality"][all4][:8], r["want_quality"][:8])
    assert r["quality"][det_only] == r["quality"][neither] == [], r["quality"]
    assert r["vad"][q_only] == r["vad"][neither] == [] and r["keys"][q_only] == r["keys"][neither] == [] and r["tones"][q_only] == r["tones"][neither] == [], r
    assert all(r["events"]) and all(r["frames"]) and r["n_events"] >= 2, r
    assert len(set(r["chunks"])) == 1 and r["chunks"][0] >= 5, r["chunks"]
    assert r["det_frames"] == [2 * r["real"]] * 4 and min(r["launches"]) > 0, r


def test_rules_refusals_and_costs_nothing_when_unused(built, tiny_model):
    """a session with the three detectors but no observer: aprilx_model_quality_stats stays (0, 0, 0.0); the same feeds with a session
    that opts in leave the other detectors' launch counts as they were; then the rules of aprilx_session_set_quality, and snapshot and
    restore refused while the observer is on"""
    r = run(tiny_model["path"], "off")
    assert r["unused"] == [0, 0, 0.0] and r["plain_info"] is None and r["plain_quality"] == 0, r
    assert r["others_launches"][0] == r["others_launches"][1] and min(r["others_launches"][0]) > 0, r["others_launches"]
    assert r["used"][0] == r["others_launches"][1][2] and r["used"][1] == r["opted_frames"] > 200 and r["opted_events"] >= 3, r
    assert r["fresh"] and r["bad"] == [-1] * 12 and r["after_bad"] == 100, r
    assert r["set"] == 0 and r["after_set"] == [50, 32124], r
    assert r["after_feed"] == -1 and r["off_after_feed"] == -1 and r["still"] == 50, r
    assert r["snapshot_refused"] == -1 and r["snapshot_when_off"], r
    assert r["restore_refused"] is not None and "line-quality" in r["restore_refused"] and r["restore_taken"], r
    assert r["frames_seen"] == r["counters"][0] > 200 and r["counters"][1] >= 6 and r["counters"][2] > 30, r
    assert r["report_times"] == [0, 500, 1000, 1500], r
    assert r["after_flush"] == 0 and r["off"] is None and r["off_launches_nothing"], r
    assert r["profiled_ms"] > 0 and r["profiled_kinds"] == [1, 2, 3, 4, 5] and r["mismatch"] == 0, r
