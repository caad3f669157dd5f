"""Session snapshot and restore (aprilx_session_snapshot / aprilx_session_restore, the batched forms).  The
uninterrupted run, the source that went on after its snapshot and the restored copy must agree exactly: callbacks, detector events,
feature rows, contexts, trie states and counters.  On the uninterrupted run every test first checks that the comparison is not empty.
Every scenario runs in a child process (tests/snapshot_worker.py)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(path, *args, env=None):
    e = dict(os.environ)
    for k in ("APRIL_PRECISION", "APRIL_GPU_DEVICES", "APRIL_RING_FRAMES"):
        e.pop(k, None)
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "snapshot_worker.py"), path] + [str(a) for a in args],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=e)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.fixture(scope="module")
def snap_model(model_dir, built):
    """tiny dimensions, weights of seed 8: the seed (of 0..11, scanned with snapshot_worker.py `scan`) with which a session WITHOUT options
    delivers FINAL and PARTIAL results after every cut below on speech_like_pcm -- the stock tiny model ends its last utterance before them"""
    from april_asr_amd import synth_model as SM
    p = str(model_dir / "snapshot_tiny8.april")
    SM.write_model(p, SM.TINY_DIMS, seed=8)
    return dict(path=p)


def not_empty(ref):
    """the reference side: there is something to compare after the cut"""
    assert ref["finals_after"] >= 1 and ref["partials_after"] >= 1, ref
    assert ref["mismatch"] == 0, ref


def check_plain(res):
    for name in ("early", "mid"):
        r = res[name]
        not_empty(r["ref"])
        assert r["bad"] == [], (name, r["bad"])
        # a non-empty audio tail and retained ring rows, fewer than a segment
        assert r["ref"]["tail_bytes"] > 0 and 0 < r["ref"]["avail"] < r["ref"]["seg"], (name, r["ref"])
    assert max(res[n]["ref"]["active_at_cut"] for n in ("early", "mid")) >= 1, res      # for one cut, an open utterance at the cut
    assert any(res[n]["ref"]["control_differs"] for n in ("early", "mid")), res                 # ... and a session without the blob goes on differently
    assert res["stats"] == [2, 2], res["stats"]                                          # one gather and one scatter per snapshot / restore


@pytest.mark.parametrize("feed", [1600, 512])
def test_plain_session(built, snap_model, feed):
    """speech_like_pcm(4 s), cut after 0.5 s + 37 samples and after 2.3 s, restored into a second session of the same engine"""
    check_plain(run(snap_model["path"], "plain", feed))


def test_other_engine(built, snap_model):
    """two engines on one GPU; the target is created while the source is live, so placement puts it on the second"""
    r = run(snap_model["path"], "engine2", env={"APRIL_GPU_DEVICES": "0,0"})
    not_empty(r["ref"])
    assert r["bad"] == [], r["bad"]
    assert r["dev0"] == [1, 0] and r["dev1"] == [0, 1], (r["dev0"], r["dev1"])


def test_other_process_ring_rebased_and_wrapped(built, snap_model, tmp_path):
    """the source runs with a 288-row ring and snapshots after 3.5 s (the ring has wrapped) to a file; the target has the default ring"""
    path = str(tmp_path / "s.snap")
    src = run(snap_model["path"], "proc_src", path, env={"APRIL_RING_FRAMES": "288"})
    assert src["ring"] == 288 and src["rows_written"] > 288 and src["avail"] > 0, src
    dst = run(snap_model["path"], "proc_dst", path)
    assert dst["finals_after"] >= 1 and dst["partials_after"] >= 1, dst
    assert dst["bad"] == [], dst["bad"]


def test_everything_opted_in(built, tiny_model):
    """an 8 kHz mu-law session with K = 4, a bias set, search options, VAD, DTMF and tones; a DTMF digit, a 1100 Hz tone and a speech
    burst each span one of the cuts"""
    res = run(tiny_model["path"], "all")
    for name in ("digit", "tone", "speech"):
        r = res[name]
        not_empty(r["ref"])
        assert r["bad"] == [], (name, r["bad"])
    assert "dtmf" in res["digit"]["kinds"][0] and "dtmf" in res["digit"]["kinds"][1], res["digit"]["kinds"]      # key down before the cut, key up after it
    assert "tone" in res["tone"]["kinds"][0] and "tone" in res["tone"]["kinds"][1], res["tone"]["kinds"]
    assert "vad" in res["speech"]["kinds"][0] and "vad" in res["speech"]["kinds"][1], res["speech"]["kinds"]
    assert max(res[n]["ref"]["bias_at_cut"] for n in ("digit", "tone", "speech")) != 0, res      # for one cut, a trie state away from the root
    assert all(res[n]["ref"]["control_differs"] for n in ("digit", "tone", "speech")), res      # a session without the blob goes on differently
    assert res["info_bad"] == [], res["info_bad"]


def test_edge_states(built, snap_model):
    """a session never fed, a session after a completed flush, a resampled session cut inside a segment"""
    res = run(snap_model["path"], "edges")
    for name in ("never_fed", "after_flush", "resampled"):
        not_empty(res[name]["ref"])
        assert res[name]["bad"] == [], (name, res[name]["bad"])
    assert res["never_fed"]["ref"]["rows_at_cut"] == 0 and res["after_flush"]["ref"]["rows_at_cut"] > 200, res
    assert res["resampled"]["in_rate"] == 8000 and res["resampled"]["segs"] >= 1 and res["resampled"]["ref"]["tail_bytes"] > 0, res["resampled"]


def test_contents_not_only_round_trips(built, snap_model):
    """a real blob read by tests/snapshot_ref.py: ctx, now_ms, chunks, real_frames, the device search state, the ring rows and the
    audio tail are what the session's own getters and the fed samples say"""
    r = run(snap_model["path"], "contents")
    assert r["bad"] == [], r["bad"]
    assert r["avail"] > 0 and r["tail"] > 0 and r["device_bytes"] % 16 == 0, r


def test_batched(built, medium_model):
    """64 sessions of the medium model with different seeds: snapshot_many, free all, restore_many; one gather and one scatter launch per engine (the
    call that only asks for the sizes launches nothing)"""
    r = run(medium_model["path"], "batched", 64)
    assert r["callbacks"] > 64 and r["distinct"] > 32, r
    assert r["same"] and r["callbacks_migrated"] == r["callbacks"] and r["mismatch"] == 0, r
    assert r["counts"]["gathers"] == 1 and r["counts"]["scatters"] == 1 and r["counts"]["other"] == 0, r["counts"]


def test_fp16_mode(built, snap_model, tmp_path):
    """the plain-session test on an fp16 engine; a blob of an fp32 engine is refused by it"""
    f16 = {"APRIL_PRECISION": "f16"}
    check_plain(run(snap_model["path"], "plain", 1600, env=f16))
    path = str(tmp_path / "f32.snap")
    run(snap_model["path"], "plain", 1600, path)
    r = run(snap_model["path"], "refuse_file", path, env=f16)
    assert r["msg"] and "precision" in r["msg"] and r["usable"], r


def test_refusals(built, tiny_model, model_dir):
    """another model, a configuration that differs in one field, a target that has been fed, a call from the session's own handler, a
    cap too small, a corrupt blob: each refused, each target able to run a normal stream afterwards"""
    from april_asr_amd import synth_model as SM
    other = str(model_dir / "snapshot_other.april")
    SM.write_model(other, SM.TINY_DIMS, params=dict(rate=8000))
    r = run(tiny_model["path"], "refusals", other)
    assert r["control"] is None, r["control"]
    for name, msg in r["config"].items():
        assert msg and "configuration differs" in msg, (name, msg)
    assert all(r["config_usable"].values()) and len(r["config_usable"]) == 4, r["config_usable"]
    assert all(r["corrupt"]), r["corrupt"]
    assert r["other_model"] and "another model" in r["other_model"], r["other_model"]
    assert r["other_config_blob"] and "configuration differs" in r["other_config_blob"], r["other_config_blob"]
    assert r["target_usable"], r
    assert r["fed"] and "fed" in r["fed"] and r["fed_open"] and "fed" in r["fed_open"], (r["fed"], r["fed_open"])
    assert r["cap"] == [-1, True], r["cap"]
    for kind in ("sync", "async"):
        n, values = r["handler_" + kind]
        assert n >= 1 and values == [-1] and r["handler_%s_after" % kind], (kind, n, values)
    assert r["source_events"] > 0


def test_serve_many_migrate(built, snap_model, tmp_path):
    """examples/serve_many --migrate S: after S feeds every stream is snapshotted, freed and restored into a new session; the printed
    per-stream results (callbacks, FINAL results, their tokens, the last FINAL text, VAD / DTMF / tone summaries) equal a run without the flag"""
    import numpy as np
    from conftest import speech_like_pcm
    exe = str(tmp_path / "serve_many")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "examples", "serve_many.cpp"), "-I", os.path.join(ROOT, "include"),
                           "-L", os.path.join(ROOT, "april_asr_amd"), "-laprilasr", "-Wl,-rpath," + os.path.join(ROOT, "april_asr_amd"), "-o", exe])
    path = str(tmp_path / "audio.raw")
    speech_like_pcm(4.0, seed=12).tofile(path)
    opts = ["--endpoint-ms", "600", "--blank-penalty", "0.5", "--vad", "--dtmf", "--tones", "--alternatives", "2"]
    outs = {}
    for name, extra in (("plain", []), ("migrate", ["--migrate", "17"]), ("migrate_lockstep", ["--migrate", "23"])):
        mode = "lockstep" if name.endswith("lockstep") else "pipelined"
        r = subprocess.run([exe, snap_model["path"], path, "8", mode] + opts + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0, r.stderr.decode()[-1000:]
        outs[name] = r.stdout.decode().splitlines()
        assert ("migrated 8 streams" in r.stderr.decode()) == bool(extra)
    assert len(outs["plain"]) == 8 and outs["migrate"] == outs["plain"] and outs["migrate_lockstep"] == outs["plain"]
    assert sum(int(ln.split()[2]) for ln in outs["plain"]) > 0, "no FINAL result in any stream"
    assert len({ln.split(" ", 1)[1] for ln in outs["plain"]}) > 1      # the streams differ
