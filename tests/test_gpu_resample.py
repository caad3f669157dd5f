"""Sessions with an input rate of their own (aprilx_session_set_input_rate): the device resampler against a float64 evaluation of the
contract and, every output bit, against the CPU model of the contract (oracle/orc_resample.c) across the
accepted rate space at 16, 44.1 and 8 kHz models; and the ingest around it -- a resampled session gives bit for bit the callbacks,
feature rows and logits of a default session fed the CPU model's conversion as it becomes available, in every feeding path (random
feed sizes, segments shorter than K / empty / of one sample, pipelined group feeds of mixed and extreme rates, one long feed, a small
staging bound, asynchronous sessions).  Every scenario runs in a child process (tests/resample_worker.py)."""
import json
import os
import subprocess
import sys

import pytest

from resample_worker import EXACT_MATRIX, EXTREME_RATES, exact_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(path, *args, **env):
    e = dict(os.environ)
    e.update({k: str(v) for k, v in env.items()})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "resample_worker.py"), path] + [str(a) for a in args],
                       env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_kernel_against_float64(built, tiny_model):
    res = run(tiny_model["path"], "kernel")
    for rate in ("8000", "11025", "22050", "32000", "44100", "48000", "96000"):
        r = res[rate]
        assert r["n_out"] == r["want"], (rate, r)
        assert r["max_diff"] <= 1 and r["exact"] >= 0.98, (rate, r)
        assert r["sq_n"] == r["sq_want"] and r["sq_max_diff"] <= 1 and r["sq_clamped"] > 0 and r["sq_clamped_equal"], (rate, r)
    assert res["tone"]["snr_db"] >= 80.0, res["tone"]
    assert res["tone"]["stop_rms"] <= 1.0, res["tone"]


@pytest.fixture(scope="module")
def rate_models(model_dir, tiny_model):
    """the tiny model at 16 kHz and at the two other model rates of the matrix (44.1 and 8 kHz)"""
    from april_asr_amd import synth_model as SM
    paths = {16000: tiny_model["path"]}
    for rate in (44100, 8000):
        p = str(model_dir / ("tiny_rate%d.april" % rate))
        SM.write_model(p, SM.TINY_DIMS, params=dict(rate=rate))
        paths[rate] = p
    return paths


# the 16 kHz row in two children (the CPU model of 383996 / 384000 Hz takes a while)
EXACT_RUNS = [(16000, EXACT_MATRIX[16000][:10]), (16000, EXACT_MATRIX[16000][10:]), (44100, EXACT_MATRIX[44100]), (8000, EXACT_MATRIX[8000])]


@pytest.mark.parametrize("sr,rates", EXACT_RUNS, ids=["16k-a", "16k-b", "44k1", "8k"])
def test_kernel_bit_exact_against_the_contract(built, rate_models, sr, rates):
    """every output of aprilx_resample equals the CPU model of the contract bit for bit: every (model rate, input rate) of the
    matrix, segment lengths 0, 1, K - 1, K, K + 1, 2K, 255 / 256 / 257 / 511 / 512 / 513 outputs and several seconds, full-scale
    noise / square wave / constants / an impulse at either end / speech-like content; aprilx_resample's own edges"""
    res = run(rate_models[sr], "exact", *rates)
    for rate in rates:
        r = res[str(rate)]
        want = [(n, kind) for n, kind, _ in exact_cases(rate, sr)]
        assert [(c[0], c[1]) for c in r["cases"]] == want, rate
        for n, kind, n_want, n_got, diff, lo, hi in r["cases"]:
            assert n_got == n_want == -((-n * r["lmk"][0]) // r["lmk"][1]), (sr, rate, n, kind, n_got, n_want)
            assert diff == 0, "%d -> %d Hz, %d samples of %s: %d outputs differ from the contract" % (rate, sr, n, kind, diff)
        noise = [c for c in r["cases"] if c[1] == "noise" and c[2] > 0]
        assert sum(c[5] for c in noise) > 0 and sum(c[6] for c in noise) > 0, (rate, "the noise must clamp on both sides")
        e = r["edges"]
        assert e["zero"] == 0, (rate, e)
        assert e["short_cap"] == -1 and e["untouched"], (rate, e)
        assert e["exact_cap"] == e["n_out"] and e["exact_cap_equal"], (rate, e)
    assert res["refused"][1] == -1, res["refused"]


@pytest.mark.parametrize("rate", [8000, 22050, 44100, 48000])
def test_session_equals_default_session_fed_converted_audio(built, tiny_model, rate):
    r = run(tiny_model["path"], "equiv", rate)
    assert r["rate"] == rate
    assert r["n_events"] > 0 and r["n_frames"] > 0 and r["n_logits"] > 0, r
    assert r["events_equal"] and r["frames_equal"] and r["logits_equal"], r


@pytest.mark.parametrize("sr,rate", [(16000, 4000), (16000, 4004), (16000, 384000), (16000, 383996), (44100, 48000), (44100, 16000),
                                     (8000, 328000)])
def test_session_at_edge_rates_equals_default_session(built, rate_models, sr, rate):
    r = run(rate_models[sr], "equiv", rate)
    assert r["rate"] == rate
    assert r["n_events"] > 0 and r["n_frames"] > 0 and r["n_logits"] > 0, r
    assert r["events_equal"] and r["frames_equal"] and r["logits_equal"], r


@pytest.mark.parametrize("sr,rate", [(16000, 48000), (16000, 4000), (16000, 384000), (16000, 383996), (44100, 16000), (8000, 328000)])
def test_short_empty_and_split_segments(built, rate_models, sr, rate):
    """segments of 5 samples (< K), empty, of 1 sample, and flushes inside a filterbank window, against the default session fed the
    CPU model's conversion of every segment"""
    r = run(rate_models[sr], "edges", rate)
    assert r["rate"] == rate
    assert r["n_frames"] > 0 and r["n_logits"] > 0, r
    assert r["events_equal"] and r["frames_equal"] and r["logits_equal"], r


def test_pipelined_group_of_extreme_rates(built, tiny_model):
    r = run(tiny_model["path"], "extremes")
    assert r["rates"] == [x or 0 for x in EXTREME_RATES * 2], r
    assert all(r["equal"]) and all(n > 0 for n in r["n_frames"]), r


def test_pipelined_group_of_mixed_rates(built, tiny_model):
    r = run(tiny_model["path"], "group")
    assert all(r["mixed_equals_single"]), r
    assert r["defaults_equal_plain"] and all(r["defaults_equal_plain"]), r
    assert r["distinct"] == 32, r


def test_long_feed_and_staging_bound(built, tiny_model):
    a = run(tiny_model["path"], "long")
    assert a["n_events"] > 0 and a["lm_chunks"] > 0, a
    assert a["one"] == a["pieces"], a
    b = run(tiny_model["path"], "long", APRIL_STAGE_LIMIT_SAMPLES=20000)
    assert b["one"] == a["one"], (a, b)


def test_async_session_and_ring_bound(built, tiny_model):
    r = run(tiny_model["path"], "asynchronous")
    assert r["async_refused"] == 0 and r["n_events"] > 0 and r["async_equals_sync"], r
    ck = r["cant_keep_up"]
    assert ck["48000"] == 0 and ck["132299"] == 0 and ck["132300"] == 1, ck
    assert ck["default_48000"] == 1, ck


def test_set_input_rate_rules(built, tiny_model):
    r = run(tiny_model["path"], "rules")
    assert r["fresh"] == 0 and r["rate_after_set"] == 48000, r
    assert r["after_feed"] == -1 and r["rate_after_refusal"] == 48000, r
    assert r["after_flush"] == 0, r
    assert r["bad_rates"] == [-1, -1, -1, -1], r
    assert r["back_to_model_rate"] == 0 and r["rate_default"] == 16000, r
    assert r["set_model_rate_equal"] and r["detour_equal"], r
    assert r["resample_launches"] > 0 and r["resample_ms"] > 0, r
