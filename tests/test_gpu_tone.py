"""Tone events per session (aprilx_session_set_tones): tone_kernel against the numpy statement of the contract
(tests/tone_ref.py), every bit of the records and of the F + 1 powers; live sessions in every ingest mode, whose events must be the
statement applied to the session's own model-rate samples; formatted streams (mu-law at 8 kHz, channel 1 of two); a twin without the
detector, which must not differ in anything; sessions with all three detectors, with one and with none in the same passes; and an engine
without an opted-in session, which must launch nothing.
Every scenario runs in a child process (tests/tone_worker.py)."""
import json
import os
import subprocess
import sys

import pytest

from tone_worker import N_SET

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(path, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tone_worker.py"), path] + [str(a) for a in args],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.fixture(scope="module")
def models(model_dir, tiny_model):
    """the tiny model (16 kHz, 512-point frames: W 512, F 64, the samples of four frames in registers), the same at 8 kHz (W 256), with
    400-sample frames that are not rounded up (W 384: 48 bins of 41.7 Hz), and at 48 kHz (W 2048, F 86: the kernel's other path, and a
    last walk of the rows that is not full)"""
    from april_asr_amd import synth_model as SM
    out = {"16k": (tiny_model["path"], 512, 64)}
    for name, params, w, f in (("8k", dict(rate=8000), 256, 64), ("n400", dict(round_pow2=0), 384, 48), ("48k", dict(rate=48000), 2048, 86)):
        p = str(model_dir / ("tone_%s.april" % name))
        SM.write_model(p, SM.TINY_DIMS, params=params)
        out[name] = (p, w, f)
    return out


@pytest.mark.parametrize("geo", ["16k", "8k", "n400", "48k"])
def test_kernel_equals_the_contract_bitwise(built, models, geo):
    """aprilx_run_tones: every run length up to twice the kernel's frames per wave plus one, 64, 65 and 257, records and all F + 1 powers;
    four runs with different options in one launch; aprilx_run_tone_decide on the edge rows"""
    path, w, f = models[geo]
    r = run(path, "kernel")
    assert (r["W"], r["F"]) == (w, f)
    assert r["calls"] == len(N_SET) + 3
    assert r["bad"] == [], r["bad"][:10]
    assert r["tonal"] >= 40, r["tonal"]                       # (the frames do hold tones)
    assert r["differ"] >= 2, r["differ"]                      # ... and the options of the four runs do change what comes out
    assert r["n_edges"] >= 14 and r["edge_bad"] == [] and r["host_bad"] == [], (r["edge_bad"], r["host_bad"])
    assert r["refusals"] == [-1, -1, -1, -1, 0], r["refusals"]


@pytest.mark.parametrize("mode", ["sync", "async", "pipe2"])
def test_live_sessions_equal_the_contract_on_their_own_samples(built, tiny_model, mode):
    """the scenario (1100 Hz, 480 + 620 Hz on and off twice, a 1400 Hz beep) with a flush inside the first pair: two PCM16 streams
    (defaults; long tones only with a long pause), a mu-law stream at 8000 Hz and a two-channel stream taking
    channel 1, EACH beside a twin without the detector (same format, same bytes, same group) whose token events, feature rows and chunk
    count must be the same: 100 ms feeds and irregular feeds with single-frame feeds"""
    chunkings = ["100ms", "irregular"]
    res = run(tiny_model["path"], "live", mode, *chunkings)
    for c in chunkings:
        r = res[c]
        assert r["mismatch"] == 0, c
        first, second = r["streams"]
        for s in (first, second):
            assert s["cku"] == 0 and s["W"] == 512, (c, s)
            assert s["n_want"] >= 4 and s["equal"], (c, s["got"], s["want"])
            assert s["frames_seen"] == s["real"] and s["tonal_frames"] == s["want_tonal"] > 0 and s["held"] is None, (c, s)
        # (the flush splits the first pair in two)
        assert first["names"] == ["cng", "busy", "busy", "busy", "sit2"] and first["info_tones"] == 5, (c, first["got"])
        assert first["closing"] == [], (c, first["got"])        # (the 400 ms of zeros a flush appends end the pair before the flush completes)
        # the long-pause stream still holds the 1100 Hz tone when the flush completes: closed at the segment's last frame
        assert second["names"][0] == "cng" and len(second["closing"]) == 1 and second["closing"][0][1] == 0, (c, second["got"])
        for f in r["formatted"]:
            assert f["cku"] == 0 and f["n_want"] >= 8 and f["equal"], (c, f["got"], f["want"])
            assert f["frames_seen"] == f["real"], (c, f)
        assert len(r["twins"]) == 4                           # the two PCM16 streams, the mu-law one, the two-channel one
        for t in r["twins"]:
            assert t["events"] and t["frames"] and t["chunks"], (c, t)
            assert t["n_events"] >= 1 and t["n_chunks"] >= 5 and t["twin_tones"] == 0 and t["twin_info"], (c, t)
        assert r["launches"] > 0 and r["tone_frames"] == r["want_tone_frames"], (c, r["tone_frames"], r["want_tone_frames"])


def test_rules_and_costs_nothing_when_unused(built, tiny_model):
    """a session with voice activity and DTMF but no tones: aprilx_model_tone_stats stays (0, 0, 0.0) (what such a pass uploads is
    tests/cpp/staging_layout_tone_test.cc's); then the rules of aprilx_session_set_tones"""
    r = run(tiny_model["path"], "off")
    assert r["unused"] == [0, 0, 0.0] and r["plain_info"] is None and r["plain_tones"] == 0, r
    assert r["fresh"] and r["bad"] == [-1] * 10 and r["after_bad"] == 6, r
    assert r["set"] == 0 and r["after_set"] == 10, r
    assert r["after_feed"] == -1 and r["off_after_feed"] == -1 and r["still"] == 10, r
    assert r["used"][0] > 0 and r["used"][1] == r["frames_seen"] > 200, r
    assert r["names"] == ["cng", "busy", "busy", "sit2"] and r["counters"][0] == 4 and r["counters"][1] >= 100, r
    assert r["after_flush"] == 0 and r["off"] is None and r["off_launches_nothing"], r
    assert r["profiled_ms"] > 0 and r["profiled_names"] == ["cng", "busy", "busy", "sit2"] and r["mismatch"] == 0, r


def test_all_three_detectors_in_the_same_passes(built, tiny_model):
    """four sessions of one group on the same 2 s (two bursts, a key inside the first and a key between them that the flush falls into,
    two tones behind them; irregular feeds): all three detectors, tones only, DTMF only, none.  The passes carry descriptors of all
    kinds, so their tone records sit behind their VAD and DTMF bytes; every detector must hear what its own numpy statement gives --
    the tone detector hears the DTMF keys too, as pairs --, and nobody's transcript may move"""
    r = run(tiny_model["path"], "all3")
    all3, tones_only, dtmf_only, neither = range(4)
    assert r["mismatch"] == 0 and r["single_frame_feeds"] >= 1, r["single_frame_feeds"]
    assert len(r["want_vad"]) >= 2 and r["vad"][all3] == r["want_vad"], (r["vad"][all3], r["want_vad"])
    assert len(r["want_keys"]) >= 4 and r["keys"][all3] == r["keys"][dtmf_only] == r["want_keys"], (r["keys"][::2], r["want_keys"])
    assert len(r["want_tones"]) >= 6 and r["tones"][all3] == r["tones"][tones_only] == r["want_tones"], (r["tones"][:2], r["want_tones"])
    assert any(e[0] == 1 and e[2] != 0 and abs(e[1] - 941) <= 20 and abs(e[2] - 1477) <= 20 for e in r["want_tones"]), r["want_tones"]      # the "#" key, as a pair
    assert r["vad"][tones_only] == r["vad"][dtmf_only] == r["vad"][neither] == [], r["vad"]
    assert r["keys"][tones_only] == r["keys"][neither] == [] and r["tones"][dtmf_only] == r["tones"][neither] == [], r
    assert all(r["events"]) and all(r["frames"]) and r["n_events"] >= 2, r
    assert len(set(r["chunks"])) == 1 and r["chunks"][0] >= 5, r["chunks"]
    assert r["det_frames"] == [r["real"], 2 * r["real"], 2 * r["real"]] and min(r["launches"]) > 0, r
