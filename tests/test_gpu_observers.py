"""The four frame observers of the front-end pass -- voice activity, DTMF, tones, line quality (DESIGN.md sections 16, 17, 18, 21 and 22) --
in every combination inside the same passes: what an observer delivers must not depend on which others run beside it.  What each
observer delivers alone is held to its numpy contract by test_gpu_vad, test_gpu_dtmf, test_gpu_tone and test_gpu_quality.
The scenario runs in a child process (tests/observers_worker.py)."""
import json
import os
import subprocess
import sys

import pytest

from observers_worker import OBSERVERS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "observers_worker.py"), path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_every_subset_of_observers_in_the_same_passes(built, tiny_model):
    """sixteen sessions of one group, one per subset of the four observers (the empty one included), on the same 1.5 s -- a burst that
    trips voice activity with a DTMF key inside it, a call-progress tone, a stretch driven into the rails, digital silence -- in 100 ms
    group feeds and a flush.  Every pass carries runs of every observer, at offsets that differ from observer to observer.  For each
    observer X: every session with X on delivers exactly the events (kind, payload, time) and shows the counters of the session with
    only X on, a session with X off delivers none; and all sixteen transcripts are equal"""
    r = run(tiny_model["path"])
    assert r["mismatch"] == 0
    for x, name in enumerate(OBSERVERS):
        alone = 1 << x
        assert len(r["events"][name][alone]) >= 1, name               # (a condition on the audio)
        assert r["info"][name][alone] is not None, name
        for mask in range(16):
            if mask >> x & 1:
                assert r["events"][name][mask] == r["events"][name][alone], (name, mask, r["events"][name][mask], r["events"][name][alone])
                assert r["info"][name][mask] == r["info"][name][alone], (name, mask, r["info"][name][mask], r["info"][name][alone])
            else:
                assert r["events"][name][mask] == [] and r["info"][name][mask] is None, (name, mask)
    assert all(r["tokens_equal"]) and r["n_token_events"] >= 1, r["tokens_equal"]
    assert len(set(r["chunks"])) == 1 and r["chunks"][0] >= 5, r["chunks"]
