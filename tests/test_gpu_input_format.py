"""Sessions with an input format (aprilx_session_set_input_format): the device decode against the numpy
statement of the contract (tests/input_format_ref.py), every bit; and the ingest around it -- a session that is fed G.711, float32
or interleaved channels gives bit for bit the callbacks, feature rows and chunk count of a plain session fed the int16 samples the
contract decodes from the same bytes, in every ingest mode, with an input rate, across flushes and under the staging limit.
Every scenario runs in a child process (tests/input_format_worker.py)."""
import json
import os
import subprocess
import sys

import pytest

from input_format_worker import COMBOS, KERNEL_FRAMES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(path, *args, **env):
    e = dict(os.environ)
    e.update({k: str(v) for k, v in env.items()})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "input_format_worker.py"), path] + [str(a) for a in args],
                       env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def all_equal(eq):
    return eq["events"] and eq["frames"] and eq["chunks"]


def test_kernel_equals_the_contract_bitwise(built, tiny_model):
    """aprilx_decode for every encoding x channels {1, 2, 3, 8} x channel {-1, 0, last} x frame counts around the kernel's 256-frame
    tile and the 64-lane wave; all 256 codes of both laws and the contract's literal values; the refusals"""
    r = run(tiny_model["path"], "kernel")
    assert r["calls"] == len(COMBOS) * len(KERNEL_FRAMES) == 44 * 9
    assert r["bad"] == [], r["bad"][:10]
    assert r["literals"] == [True] * 5, r["literals"]
    assert r["refusals"] == [-1, -1, -1, -1, 0, 4], r["refusals"]


@pytest.mark.parametrize("mode", ["sync", "async", "pipe2"])
def test_live_sessions_equal_pcm16_sessions(built, tiny_model, mode):
    """one pair of sessions per (encoding, channels, channel); the formatted sessions are fed in one group call so that many
    descriptors with different byte offsets share a pass, their PCM16 twins through the PCM16 entry points: 100 ms feeds, irregular feeds
    with single-frame feeds, one feed of the whole signal; a flush in the middle and audio after it; and the decode counters move"""
    chunkings = ["100ms", "irregular", "whole"]
    res = run(tiny_model["path"], "live", mode, *chunkings)
    fed = 0
    for c in chunkings:
        r = res[c]
        assert r["cku"] == 0 and r["mismatch"] == 0, (c, r["cku"], r["mismatch"])
        assert [f is not None for f in r["formats"]] == [combo != ("s16", 1, 0) for combo in COMBOS]
        # (an empty transcript must not pass vacuously)
        assert min(r["tokens"]) >= 1 and min(r["chunks"]) >= 10, (c, r["tokens"], r["chunks"])
        bad = [COMBOS[i] for i, e in enumerate(r["equal"]) if not all_equal(e)]
        assert not bad, (c, bad, [e for e in r["equal"] if not all_equal(e)][:4])
        fed += r["fed"]
        assert r["launches"] > 0 and r["frames"] >= fed > 0, (c, r["launches"], r["frames"], fed)


def test_with_an_input_rate(built, tiny_model):
    """mu-law, 2 channels, channel 1 at 8000 Hz and F32 downmix at 44100 Hz against PCM16 sessions at those rates fed the decoded samples"""
    r = run(tiny_model["path"], "rates")
    assert r["mismatch"] == 0
    for name, rate, fmt in (("mulaw8k", 8000, ["mulaw", 2, 1]), ("f32_44k1", 44100, ["f32", 2, -1])):
        x = r[name]
        assert x["rate"] == rate and x["fmt"] == fmt and x["other_order"] == [rate, fmt], x
        assert x["tokens"] >= 1 and x["chunks"] >= 10, x
        assert all_equal(x), x


def test_rules(built, tiny_model):
    r = run(tiny_model["path"], "rules")
    assert r["fresh_none"] is None and r["set"] == 0 and r["read"] == ["mulaw", 2, 1], r
    assert r["bad"] == [-1] * 6 and r["after_bad"] == ["mulaw", 2, 1], r
    assert r["partial"] == -1 and r["settable_after_partial"] == 0, r              # nothing was queued
    assert r["after_feed"] == -1 and r["after_refusal"] == ["mulaw", 2, 1], r       # refused after a feed ...
    assert r["tokens"] >= 1 and r["chunks"] >= 10 and all_equal(r["equal"]), r      # feed_bytes, then aas_feed_pcm16 with raw bytes
    assert r["after_flush"] == 0 and r["read_after_flush"] == ["alaw", 1, 0], r     # ... accepted after a completed flush
    assert r["default_struct"] == 0 and r["default_reads"] is None and r["null"] == 0, r
    assert r["dropped_still_settable"] == 0, r
    assert r["group_partial"] == -1 and r["group_nothing_queued"] == 0, r
    assert r["getter_bad_args"] == [-1, -1] and r["mismatch"] == 0, r


def test_costs_nothing_when_unused(built, tiny_model):
    r = run(tiny_model["path"], "plain")
    assert r["chunks"] >= 10 and r["default_equal"], r
    assert r["plain"] == [0, 0, 0.0], r                      # plain sessions (and {S16, 1, 0}): no launch, no frame
    launches, frames, ms = r["profiled"]
    assert launches > 0 and frames >= 2 * 16000 and ms > 0, r


def test_staging_limit(built, tiny_model):
    """2 s of F32 with 8 channels (1 MB) in one call with the limit at its minimum of 4096 samples: passes of a few frames each"""
    r = run(tiny_model["path"], "limit", APRIL_STAGE_LIMIT_SAMPLES=4096)
    assert r["limit"] == "4096" and r["bytes"] == 2 * 16000 * 32, r
    assert r["mismatch"] == 0 and r["tokens"] >= 1 and r["chunks"] >= 10, r
    assert all_equal(r) and r["launches"] > 8, r
