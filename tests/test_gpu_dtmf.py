"""DTMF digits per session (aprilx_session_set_dtmf): dtmf_kernel against the numpy statement of the contract
(tests/dtmf_ref.py), every bit of the codes and the nine powers; live sessions in every ingest mode, whose events must be the statement
applied to the session's own samples; formatted streams (mu-law at 8 kHz, channel 1 of two) that must give the same keys; a twin
without the detector, which must not differ in anything; sessions with both detectors, with one and with none in the same passes; and
an engine without an opted-in session, which must launch nothing.
Every scenario runs in a child process (tests/dtmf_worker.py)."""
import json
import os
import subprocess
import sys

import pytest

from dtmf_worker import N_SET

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(path, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dtmf_worker.py"), path] + [str(a) for a in args],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.fixture(scope="module")
def models(model_dir, tiny_model):
    """the tiny model (16 kHz, 512-point frames: Wd 256), the same at 8 kHz (Wd 128), and with 13 ms frames that are not rounded up
    (Wd 208: a ragged last chain; a model file holds whole milliseconds, so 12.5 ms -- Wd 200 -- exists on the CPU side only), and at
    48 kHz (Wd 768: beyond the windows whose table values a lane keeps in registers, the kernel's other path)"""
    from april_asr_amd import synth_model as SM
    out = {"16k": (tiny_model["path"], 256)}
    for name, params, wd in (("8k", dict(rate=8000), 128), ("n208", dict(round_pow2=0, length_ms=13), 208), ("48k", dict(rate=48000), 768)):
        p = str(model_dir / ("dtmf_%s.april" % name))
        SM.write_model(p, SM.TINY_DIMS, params=params)
        out[name] = (p, wd)
    return out


@pytest.mark.parametrize("geo", ["16k", "8k", "n208", "48k"])
def test_kernel_equals_the_contract_bitwise(built, models, geo):
    """aprilx_run_dtmf: run lengths around a workgroup's waves and around one pass, codes and all nine powers; four runs with different
    options in one launch; aprilx_run_dtmf_decide on the exact ties"""
    path, wd = models[geo]
    r = run(path, "kernel")
    assert r["Wd"] == wd
    assert r["calls"] == len(N_SET) + 3
    assert r["bad"] == [], r["bad"][:10]
    assert r["tones"] >= 40, r["tones"]                       # (the frames do hold digits)
    assert r["differ"] >= 3, r["differ"]                      # ... and the options of the four runs do change what comes out
    assert r["n_ties"] >= 14 and r["tie_bad"] == [], r["tie_bad"]
    assert r["refusals"] == [-1, -1, -1, -1, 0], r["refusals"]


@pytest.mark.parametrize("mode", ["sync", "async", "pipe2"])
def test_live_sessions_equal_the_contract_on_their_own_samples(built, tiny_model, mode):
    """the key string with a 200 ms key that the first flush falls into: two PCM16 streams (defaults; long keys only with a long pause),
    a mu-law stream at 8000 Hz and a two-channel stream taking channel 1, EACH of the four beside a twin without the detector (same
    format, same bytes, same group) whose token events, feature rows and chunk count must be the same: 100 ms feeds, irregular
    feeds with single-frame feeds, and each segment in one feed"""
    chunkings = ["100ms", "irregular", "whole"]
    res = run(tiny_model["path"], "live", mode, *chunkings)
    for c in chunkings:
        r = res[c]
        assert r["mismatch"] == 0, c
        first, second = r["streams"]
        for s in (first, second):
            assert s["cku"] == 0 and s["Wd"] == 256, (c, s)
            assert s["n_want"] >= 4 and s["equal"], (c, s["got"], s["want"])
            assert s["frames_seen"] == s["real"] and s["tone_frames"] == s["want_tone"] > 0 and s["held"] == "", (c, s)
        assert first["digits"] == r["want_digits"] and first["info_digits"] == len(r["want_digits"]) and not first["closing"], (c, first["digits"])
        # the long-pause stream still holds the 9 when the first flush completes: closed at the segment's last frame, found again afterwards
        assert second["digits"] == "99" and second["off_frames"] == 60 and second["closing"], (c, second["got"])
        for f in r["formatted"]:
            assert f["cku"] == 0 and f["digits"] == r["want_digits"] and f["kinds"], (c, f["got"])
            assert f["worst_ms"] <= r["on_ms"], (c, f["worst_ms"])
            assert f["frames_seen"] == f["real"], (c, f)
        assert len(r["twins"]) == 4                           # the two PCM16 streams, the mu-law one, the two-channel one
        for t in r["twins"]:
            assert t["events"] and t["frames"] and t["chunks"], (c, t)
            assert t["n_events"] >= 2 and t["n_chunks"] >= 5 and t["twin_keys"] == 0 and t["twin_info"], (c, t)
        assert r["launches"] > 0 and r["dtmf_frames"] == r["want_dtmf_frames"], (c, r["dtmf_frames"], r["want_dtmf_frames"])


def test_rules_and_costs_nothing_when_unused(built, tiny_model):
    r = run(tiny_model["path"], "rules")
    assert r["unused"] == [0, 0, 0.0] and r["plain_info"] is None, r
    assert r["fresh"] and r["bad"] == [-1] * 11 and r["after_bad"] == 2, r
    assert r["set"] == 0 and r["after_set"] == 4, r
    assert r["after_feed"] == -1 and r["off_after_feed"] == -1 and r["still"] == 4, r
    assert r["used"][0] > 0 and r["used"][1] == r["frames_seen"] > 80, r
    assert r["digits_found"][0] == "159D" and r["digits_found"][1] == 4 and r["digits_found"][2] >= 16, r
    assert r["after_flush"] == 0 and r["counters_restart"] == [0, 0, r["frames_seen"], 2], r
    assert r["off"] is None and r["off_launches_nothing"], r
    assert r["profiled_ms"] > 0 and r["profiled_digits"] == "159D" and r["mismatch"] == 0, r


def test_both_detectors_in_the_same_passes(built, tiny_model):
    """four sessions of one group on the same 1.5 s (two bursts, a key inside the first and a key between them that the flush falls into;
    irregular feeds): VAD and DTMF, VAD only, DTMF only, neither.  The passes carry descriptors of both kinds, so their DTMF bytes sit
    behind their VAD bytes; the session with both must hear what the single-detector sessions hear, which is what the two numpy
    statements give, and nobody's transcript may move"""
    r = run(tiny_model["path"], "both")
    both, vad_only, dtmf_only, neither = range(4)
    assert r["mismatch"] == 0 and r["single_frame_feeds"] >= 1, r["single_frame_feeds"]
    assert len(r["want_vad"]) >= 2 and r["vad"][both] == r["vad"][vad_only] == r["want_vad"], (r["vad"][:2], r["want_vad"])
    assert len(r["want_keys"]) >= 4 and r["keys"][both] == r["keys"][dtmf_only] == r["want_keys"], (r["keys"][::2], r["want_keys"])
    assert r["vad"][dtmf_only] == r["vad"][neither] == [] and r["keys"][vad_only] == r["keys"][neither] == [], r
    assert all(r["events"]) and all(r["frames"]) and r["n_events"] >= 2, r
    assert len(set(r["chunks"])) == 1 and r["chunks"][0] >= 5, r["chunks"]
    # two sessions opted into each detector: the same frames under both kernels
    assert r["vad_frames"] == r["dtmf_frames"] == 2 * r["real"] and min(r["launches"]) > 0, r
