"""The host scheduler under sanitizers ("-fsanitize=thread,address on the host scheduler").

tests/sched_harness/ builds the REAL host runtime -- csrc/session.cc (two flights in the air, spin waits, work / done sequence
counters, lent buffers), csrc/april_api.cc (the C ABI), csrc/host_pool.h, the loader -- host-only against a fake engine
(fake_engine.cc: asynchronous flight completion after a random delay, records visible only once a flight has completed, small
rings, decisions by a copy of the product's own state machine) and drives it through the C ABI in the scenarios of
test_gpu_pipeline.py / test_gpu_concurrency.py: lock-step, pipelined and asynchronous ingest with identical callbacks, eight client
threads with their own sessions, session churn beside streaming sessions, frees from inside handlers, queue overflow, irregular and
long feeds.  Once with -fsanitize=thread, once with -fsanitize=address,undefined; any report, inconsistency, replay mismatch or
hang fails.  Reference threading contract: src/april_session.c:479-493,567-585, src/audio_provider.c:25-40."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "sched_harness", "build.sh")


def _build(tmp, name, flags):
    out = os.path.join(str(tmp), name)
    r = subprocess.run(["bash", BUILD, flags, out], capture_output=True, timeout=900)
    if r.returncode != 0 and b"sanitizer" in r.stderr.lower() and b"unsupported" in r.stderr.lower():
        pytest.skip("toolchain without this sanitizer runtime")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return out


def _run(exe, model, **env):
    e = dict(os.environ, APRIL_LOG_LEVEL="NONE", TSAN_OPTIONS="halt_on_error=1 second_deadlock_stack=1", ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    e.update({k: str(v) for k, v in env.items()})
    r = subprocess.run([exe, model], env=e, capture_output=True, timeout=600)
    out = r.stdout.decode() + r.stderr.decode()
    assert "ThreadSanitizer" not in out and "AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
    assert r.returncode == 0 and "HARNESS ok" in out, out[-4000:]          # (the driver itself checks replay_mismatch == 0)
    m = re.search(r"HARNESS ok: .* (\d+) steps \((\d+) layer-major / (\d+) wavefront\), .* ref digest ([0-9a-f]{16})$", out, re.M)
    assert m, out[-4000:]
    return dict(steps=int(m.group(1)), lm_steps=int(m.group(2)), wave_steps=int(m.group(3)), digest=m.group(4))


def _run_stepping_paths(exe, model, **env):
    """The knobs that route chunk steps: without the feed wavefront, without the layer-major path, and without both -- every step
    is then a chunk step of one chunk per session (sub-batches included) -- also with flights that fill up after one step."""
    runs = [_run(exe, model, APRIL_WAVE_MIN_CHUNKS=0, **env), _run(exe, model, APRIL_LM_MIN_CHUNKS=0, **env)]
    assert runs[0]["wave_steps"] == 0 and runs[1]["lm_steps"] == 0
    for extra in ({}, dict(FAKE_STEP_CAP=1)):
        r = _run(exe, model, APRIL_WAVE_MIN_CHUNKS=0, APRIL_LM_MIN_CHUNKS=0, **dict(env, **extra))
        assert r["lm_steps"] == 0 and r["wave_steps"] == 0 and r["steps"] > 0, r      # "0 layer-major / 0 wavefront", and it stepped
        runs.append(r)
    return runs


def _assert_one_digest(runs):
    """Every single-engine run of one build delivers the same callbacks in the driver's reference pass (one FNV digest over all of
    them): the fake engine decides from the samples alone, so neither the stepping path that served a chunk, nor the flight it
    went into, nor the pipelining or spinning around it may show.  (The three-engine run spreads the sessions over three fake
    engines; it is checked by the driver's own comparisons and left out of this one.)"""
    assert len({r["digest"] for r in runs}) == 1, runs


@pytest.fixture(scope="module")
def harness_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("sched_harness")


def test_scheduler_under_thread_sanitizer(harness_dir, tiny_model):
    exe = _build(harness_dir, "harness_tsan", "-fsanitize=thread")
    runs = [_run(exe, tiny_model["path"])]
    runs.append(_run(exe, tiny_model["path"], FAKE_STEP_CAP=1))                      # every flight fills up: follow-up flights of one tick
    runs.append(_run(exe, tiny_model["path"], APRIL_PIPELINE=1))                     # one flight at a time
    runs.append(_run(exe, tiny_model["path"], FAKE_DELAY_US=0, FAKE_DELAY_US_MAX=5, FAKE_STEP_CAP=2))      # flights complete at once
    runs.append(_run(exe, tiny_model["path"], APRIL_SPIN_STEP_US=0, APRIL_SPIN_WAIT_US=0))                 # no spinning: every hand-over through the condition variables
    _run(exe, tiny_model["path"], APRIL_GPU_DEVICES="0,0,0")          # three engines = three stepping threads behind one model; least-loaded placement from client threads
                                                                         # (found in round 5: Engine::live_slots() read the slot count without the lock -> now atomic)
    runs += _run_stepping_paths(exe, tiny_model["path"])
    _assert_one_digest(runs)


def test_scheduler_under_address_and_ub_sanitizers(harness_dir, tiny_model):
    exe = _build(harness_dir, "harness_asan", "-fsanitize=address,undefined -fno-sanitize-recover=undefined")
    runs = [_run(exe, tiny_model["path"]), _run(exe, tiny_model["path"], FAKE_STEP_CAP=1, APRIL_HOST_THREADS=8)]
    runs += _run_stepping_paths(exe, tiny_model["path"])
    _assert_one_digest(runs)
