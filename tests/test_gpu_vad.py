"""Voice activity per session (aprilx_session_set_vad): vad_kernel against the numpy statement of the contract
(tests/vad_ref.py), every bit; live sessions in every ingest mode, whose events must be the statement applied to the session's own real
feature rows; a twin without the detector, which must not differ in anything; and an engine without an opted-in session, which must
launch nothing.  Every scenario runs in a child process (tests/vad_worker.py)."""
import json
import os
import subprocess
import sys

import pytest

from vad_worker import NB_SET, N_SET

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(path, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "vad_worker.py"), path] + [str(a) for a in args],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_kernel_equals_the_contract_bitwise(built, tiny_model):
    """aprilx_run_vad: bands of 1 .. 80 bins x run lengths around the 16-frame pass and the 256-frame tile, bytes, energies and final
    state; eight runs with different options in one launch, two of them wrapping the ring; their states carried into a second launch;
    pad-value rows, -0.0 and exact threshold ties among the rows"""
    r = run(tiny_model["path"], "kernel")
    assert r["calls"] == len(NB_SET) * len(N_SET) + 2
    assert r["bad"] == [], r["bad"][:10]
    assert r["tie_frames"] == 2 * sum(1 for n in N_SET if n >= 6), r["tie_frames"]      # d == thr_on occurred, and was not speech
    assert r["speech_runs"] >= 10, r["speech_runs"]
    assert r["refusals"] == [-1, -1, -1, -1, 0], r["refusals"]


@pytest.mark.parametrize("mode", ["sync", "async", "pipe2"])
def test_live_sessions_equal_the_contract_on_their_own_rows(built, tiny_model, mode):
    """three streams of the burst signal (six bursts, a flush inside the fifth) with different options and a mu-law stream at 8000 Hz,
    beside twins without the detector: 100 ms feeds, irregular feeds with single-frame feeds, and each segment in one feed"""
    chunkings = ["100ms", "irregular", "whole"]
    res = run(tiny_model["path"], "live", mode, *chunkings)
    for c in chunkings:
        r = res[c]
        assert r["mismatch"] == 0, c
        assert len(r["streams"]) == 4
        assert [s["long_hangover"] for s in r["streams"]] == [True, False, False, True]
        for s in r["streams"]:
            assert s["cku"] == 0 and s["band"] == s["want_band"], (c, s)
            assert s["segments"] >= 4, (c, s["segments"], s["want"])                 # (an empty result must not pass)
            assert s["equal"], (c, s["got"], s["want"])
            assert s["frames_seen"] == s["real"] and s["info_segments"] == s["segments"], (c, s)
            assert s["speech_frames"] == s["want_speech"] > 0 and s["in_speech"] == 0, (c, s)
            # the flush inside the fifth burst: streams whose hangover outlasts the flush zeros get the closing SPEECH_END at the
            # segment's last frame; every stream finds speech again afterwards, from a reset state
            assert s["closing"] == s["long_hangover"] and s["after"] >= 1, (c, s["got"])
        for t in r["twins"]:
            assert t["events"] and t["frames"] and t["chunks"], (c, t)
            assert t["tokens"] >= 1 and t["n_chunks"] >= 10 and t["twin_vad"] == 0, (c, t)
        assert r["launches"] > 0 and r["vad_frames"] == r["want_vad_frames"] * (chunkings.index(c) + 1), (c, r["vad_frames"], r["want_vad_frames"])


def test_rules_and_costs_nothing_when_unused(built, tiny_model):
    r = run(tiny_model["path"], "rules")
    assert r["unused"] == [0, 0, 0.0] and r["plain_info"] is None and r["plain_frames_seen"] > 200, r
    assert r["fresh"] and r["bad"] == [-1] * 9 and r["after_bad"] == 5, r
    assert r["set"] == 0 and r["after_set"] == 8, r
    assert r["after_feed"] == -1 and r["off_after_feed"] == -1 and r["still"] == 8, r
    assert r["used"][0] > 0 and r["used"][1] == r["frames_seen"] > 200, r
    assert r["after_flush"] == 0 and r["counters_restart"] == [0, 0, r["frames_seen"]], r
    assert r["off"] is None and r["off_launches_nothing"] and r["frames_seen_runs_on"] > r["frames_seen"], r
    assert r["profiled_ms"] > 0 and r["events"][0] >= 2 and r["events"][1] >= 2 and r["mismatch"] == 0, r
