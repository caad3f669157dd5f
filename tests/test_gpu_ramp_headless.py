"""Ramp merge with the deferred enqueue (APRIL_RAMP_MERGE=1): the latch kernel reports its decision to the host, and
the host enqueues the hosted feed's layer graph WITHOUT the head steps the chain in front has run -- instead of enqueueing it early with
its head behind a device flag (APRIL_RAMP_MERGE=3, the form before).  Neither may change a single callback: the same sessions and audio
go through the pipelined group feed at depth 2 with APRIL_RAMP_MERGE = 0, 1 and 3 (tests/ramp_headless_worker.py, one process per
scenario); every token, log-probability (bit for bit), flag and time must agree and replay_mismatch must stay 0.

Model, session count and feed count: those of tests/test_gpu_ramp_merge.py (aprilv0 dimensions, 256 sessions, 40 feeds; the comments
there give the reasons)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEEDS, NSESS = 40, 256
# Hosting depends on whether the next feed's front end is through when the latch looks, i.e. on host timing, in both forms alike.  The
# form before hosted 77, 78, 80, 80, 78 and 78, 80, 78, 78, 80 of 82 offered feeds in two jobs of five runs of this shape (LAB_NOTES.md,
# "Ramp merge", second and third measurement): a spread of 3 from run to run with nothing changed.  That spread is the slack.
HOSTED_SLACK = 3
STEP_TIMEOUT = 300          # seconds per worker process (a whole scenario takes a few; this only ends a run that has stopped)


def run(path, scenario, modes, extra_env=None, noclose=False):
    e = dict(os.environ, APRIL_MAX_SESSIONS="512", APRIL_MAX_BATCH="2048", **(extra_env or {}))
    cmd = [sys.executable, os.path.join(ROOT, "tests", "ramp_headless_worker.py"), path, scenario, str(NSESS), str(FEEDS), modes]
    r = subprocess.run(cmd + (["noclose"] if noclose else []), env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=STEP_TIMEOUT)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    run.last_stderr = r.stderr.decode(errors="replace")
    out, closed = {}, []
    for ln in r.stdout.decode().splitlines():
        f = ln.split()
        if ln.startswith("MODE"):
            out[f[1]] = dict(digest=f[2], chunks=int(f[3]), mismatch=int(f[4]), calls=int(f[5]), hosted=int(f[6]), eligible=int(f[7]),
                             headless=int(f[8]), settled_wait=int(f[9]), settled_other=int(f[10]))
            print(scenario, extra_env, f[1], out[f[1]])
        elif ln.startswith("CLOSED"):
            closed.append(f[1])
    return closed if noclose else out


def check_identity(out):
    ref = out["0"]
    assert ref["chunks"] > 0 and ref["calls"] > 0
    for mode, got in out.items():
        assert got["mismatch"] == 0, (mode, got)
        assert got["chunks"] == ref["chunks"] and got["digest"] == ref["digest"], "callbacks differ: %s %r vs %r" % (mode, got, ref)
    assert ref["hosted"] == 0 and ref["eligible"] == 0 and ref["headless"] == 0
    for mode, got in out.items():
        if mode != "1":
            assert got["headless"] == 0 and got["settled_wait"] == 0 and got["settled_other"] == 0, (mode, got)


def check_settled(on):
    """every offered feed's layer graph was deferred and every deferral was settled; a headless graph went out exactly where the device hosted"""
    assert on["settled_wait"] + on["settled_other"] == on["eligible"], on
    assert on["headless"] == on["hosted"], on


def test_steady_feeds_one_digest_headless_equals_hosted(built, v0_model):
    """100 ms feeds (2 / 3 chunks alternate).  Not vacuous: most feeds are offered, and the deferred form hosts what the guarded form hosts.

    The last assertion (hosted with `=1` >= hosted with `=3` - HOSTED_SLACK) is NOT met in every run; the slack stays what the parent's
    counts give.  Measured, hosted of offered, `=1` against `=3` in the same process, four runs: 32 of 33 against 34 of 35, 33 of 35
    against 32 of 33, 33 of 35 against 33 of 35 and 30 of 33 against 34 of 35 (the last one fails: 30 < 34 - 3).  Two of the missing
    feeds are feeds that were not OFFERED (33 instead of 35: a run's first split feeds, in either form); among the offered ones the
    deferred form left 1, 2, 2 and 3 un-hosted, the guarded form 1, 1, 2 and 1."""
    out = run(v0_model["path"], "ms100", "0,1,3")
    assert sorted(out) == ["0", "1", "3"]
    check_identity(out)
    on, guarded = out["1"], out["3"]
    check_settled(on)
    assert guarded["eligible"] >= FEEDS // 2 and guarded["hosted"] >= (guarded["eligible"] + 1) // 2, guarded
    assert on["eligible"] >= FEEDS // 2, on
    assert on["hosted"] >= guarded["hosted"] - HOSTED_SLACK, (on, guarded)


def test_sessions_join_and_leave(built, v0_model):
    """every fourth feed eight sessions close and eight new ones open.  The digest stays, every deferral is settled, and some are settled
    by an entry other than the flight wait.

    The last assertion depends on host timing and is NOT met in every run; it is left as it is asked for.  The scenario drains the pipeline
    before sessions leave, so the slot resets find nothing deferred; what is left for "another entry" is a launch that finds the latch's
    report already there (a late host) and a second step of the same flight (new sessions are a chunk behind the others), and both need
    the feed in front to have been offered.  Measured, 256 sessions, 40 feeds, three runs: 22 / 23 / 23 offered, 16 / 23 / 17 settled by
    the flight wait and 6 / 0 / 6 by another entry.  Hosted: 8 of 22, 9 of 23 and 9 of 23, against 12 of 22, 13 of 22 and 12 of 25 with
    APRIL_RAMP_MERGE=3 in the same runs (LAB_NOTES.md, "Ramp merge", fourth measurement)."""
    out = run(v0_model["path"], "churn", "0,1,3")
    assert sorted(out) == ["0", "1", "3"]
    check_identity(out)
    on = out["1"]
    check_settled(on)
    assert on["eligible"] > 0, on
    assert on["settled_other"] > 0, on


def test_graph_cache_eviction(built, v0_model):
    """APRIL_GRAPH_CACHE_CAP=2: four plans (2 and 3 chunks, two parities) take turns in a cache of two, so the cache is emptied again and
    again (every emptying drains the streams, which settles whatever is deferred first).  Measured at this cap: the plans evict each other
    before a shape reaches its second use, so no feed is captured, split or offered (0 eligible) -- what the case pins is the digest."""
    out = run(v0_model["path"], "ms100", "0,1", extra_env={"APRIL_GRAPH_CACHE_CAP": "2"})
    assert sorted(out) == ["0", "1"]
    check_identity(out)
    check_settled(out["1"])


def test_eviction_with_deferrals_in_play(built, v0_model):
    """The `switch` scenario (100 ms feeds, then 160 ms, then 100 ms again: 2 / 3, 4, 2 / 3 chunks) with APRIL_GRAPH_CACHE_CAP=4: the four
    plans of the 100 ms feeds (two chunk counts, two parities) fill the cache, are captured and host; the first 4-chunk feed finds the
    cache full and empties it -- plans, graphs, the headless ones among them -- behind a steady series of deferred feeds, and so does the
    way back.  Every emptying drains the streams first, which settles what is deferred while its graphs still exist.  Not vacuous:
    the library's log shows the emptyings, feeds are offered and hosted around them, every deferral is settled, the digest is that of `=0`."""
    out = run(v0_model["path"], "switch", "0,1", extra_env={"APRIL_GRAPH_CACHE_CAP": "4", "APRIL_LOG_LEVEL": "INFO"})
    assert sorted(out) == ["0", "1"]
    emptied = run.last_stderr.count("feed wavefront plans emptied")
    print("plan cache emptied", emptied, "times in the two runs")
    assert emptied >= 4, "each of the two runs empties the plan cache at least twice (to 4 chunks and back): %d" % emptied
    check_identity(out)
    on = out["1"]
    check_settled(on)
    assert on["eligible"] > 0 and on["hosted"] > 0, on


def test_close_right_after_the_last_feed(built, v0_model):
    """no drain, no flush: sessions and model are closed while the last feeds are in the air, the last one possibly with its layer graph
    deferred.  The worker must come back (its time limit is the check for a hang) with exit status 0.  What settles a deferral that is
    still open then is most likely not the engine's destructor: the stepping thread's own flight wait usually comes first, and closing
    256 sessions resets their slots in one batch on the layer stream, which settles too.  The case checks the end, not which entry got there."""
    assert run(v0_model["path"], "ms100", "1", noclose=True) == ["1"]
