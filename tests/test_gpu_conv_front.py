"""The conv front end (conv12_kernel, conv12_wide_kernel, conv_weight_transpose_kernel, launch_conv_embed) against a float64
reference, one launch at a time, over the geometries the loader lets through -- and three whole models at geometries other than the
product's (mel 40, mel 128, an 11-frame segment) against the CPU oracle, at the bars of tests/test_gpu_parity.py.

aprilx_run_conv_front (csrc/conv_debug_api.cc) runs ONE launch the way the engine launches it; tests/conv_ref.py states what it
must compute, a tolerance per element and which elements must stay unwritten.  One worker process per value of APRIL_CONV_WIDE_MIN
(-1: the grouped form always; 0: the many-chunk form wherever it exists; the default: from 48 chunks), each under a time limit of
its own; a worker that ends on any status but 0 (a signal, an abort, its time limit, a failed HIP call) fails every later test of the
module at once, without another GPU process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_front_worker as W      # noqa: E402
from conftest import speech_like_pcm      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 120
STATE = {"dead": None, "results": {}}


def run_worker(knobs):
    if STATE["dead"]:
        pytest.fail("not started: " + STATE["dead"])
    env = {k: v for k, v in os.environ.items() if k != "APRIL_CONV_WIDE_MIN"}
    env.update(W.KNOB_SETS[knobs])
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.join(ROOT, "tests", "conv_front_worker.py"), knobs],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out = r.stdout.decode()
    lines = [ln for ln in out.splitlines() if ln.startswith("CASE ")]
    print("\n".join(lines))
    if r.returncode != 0:
        # the card may be in no state to take another process
        STATE["dead"] = "the worker of knob set %r ended with status %d" % (knobs, r.returncode)
        pytest.fail("worker %r: status %d\n%s\n%s" % (knobs, r.returncode, "\n".join(lines[-5:]), r.stderr.decode()[-2000:]))
    res = [ln for ln in out.splitlines() if ln.startswith("RESULT ")]
    assert res, out[-2000:]
    STATE["results"][knobs] = json.loads(res[-1][7:])
    return STATE["results"][knobs]


@pytest.mark.parametrize("knobs", list(W.KNOB_SETS))
def test_every_launch_matches_the_float64_reference(built, knobs):
    results = run_worker(knobs)
    assert len(results) == len(W.cases(knobs)), "the worker stopped early"
    for form, name in ((W.GROUPED, "grouped"), (W.WIDE, "many-chunk")):
        ratios = [r["ratio"] for r in results if r["form"] == form and r["ratio"] is not None]
        if ratios:
            print("WORST %s, %s form: err / tol = %.3g over %d cases" % (knobs, name, max(ratios), len(ratios)))
    bad = [r for r in results if not r["ok"]]
    assert not bad, "%d of %d cases fail:\n%s" % (len(bad), len(results), "\n".join("%s: %s" % (r["name"], r["why"]) for r in bad[:40]))


def test_the_two_forms_give_the_same_bytes(built):
    """Wherever the many-chunk form ran, the grouped form's output of the same case has the same digest."""
    if STATE["dead"]:
        pytest.fail("not started: " + STATE["dead"])
    assert set(STATE["results"]) == set(W.KNOB_SETS), "a worker did not finish"
    grouped = {r["name"]: r for r in STATE["results"]["grouped"]}
    compared, differ = 0, []
    for knobs in ("wide", "default"):
        for r in STATE["results"][knobs]:
            if r["rc"] != 0:
                continue
            g = grouped.get(r["name"])
            assert g is not None and g["rc"] == 0 and g["form"] == W.GROUPED, r["name"]
            compared += r["form"] == W.WIDE
            if g["digest"] != r["digest"]:
                differ.append("%s (%s, form %d)" % (r["name"], knobs, r["form"]))
    assert compared >= 20 and not differ, differ


def test_the_cases_that_ran_cover_every_path(built):
    if STATE["dead"]:
        pytest.fail("not started: " + STATE["dead"])
    assert set(STATE["results"]) == set(W.KNOB_SETS), "a worker did not finish"
    ran = [r for rs in STATE["results"].values() for r in rs if r["rc"] == 0]
    missing = W.missing_paths(ran)
    assert not missing, "no case ran on: " + ", ".join(missing)


# ------------------------------------------------------------------ whole models at other geometries
@pytest.fixture(scope="module", params=[m[0] for m in W.MODEL_DIMS])
def other_model(request, model_dir, built):
    import april_asr_amd as A
    from april_asr_amd import synth_model as SM
    from oracle import orc_py as O
    if STATE["dead"]:
        pytest.fail("not started: " + STATE["dead"])
    name, dims, step = next(m for m in W.MODEL_DIMS if m[0] == request.param)
    path = str(model_dir / ("front_%s.april" % name))
    SM.write_model(path, dims, seed=11, params=dict(step=step))
    gm, om = A.Model(path), O.Model(path)
    yield dict(gm=gm, om=om, dims=dims, step=step)
    gm.close(); om.close()


def test_other_geometry_fbank_bit_exact(other_model):
    from oracle import orc_py as O
    gm, dims = other_model["gm"], other_model["dims"]
    n = gm.dims.fft_size
    rng = np.random.RandomState(1)
    pcm = np.concatenate([O.lcg_pcm16_fast(n * 16, seed=99).reshape(16, n), rng.randint(-300, 300, size=(8, n)).astype(np.int16), np.zeros((2, n), np.int16)])
    got = gm.run_fbank(pcm)
    fb = O.OrcFbank(nbins=dims["mel"], seg_count=dims["seg"], seg_step=other_model["step"])
    want = np.stack([fb.frame(pcm[i].astype(np.float32) / np.float32(32768.0)) for i in range(pcm.shape[0])])
    assert got.shape == want.shape == (pcm.shape[0], dims["mel"])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "max |diff| = %g" % np.abs(got - want).max()


def test_other_geometry_encoder_matches_oracle(other_model):
    gm, om = other_model["gm"], other_model["om"]
    d = gm.dims
    assert (d.seg, d.mel) == (other_model["dims"]["seg"], other_model["dims"]["mel"])
    rng = np.random.RandomState(5)
    n = 3
    x = rng.uniform(-16, 8, size=(n, d.seg, d.mel)).astype(np.float32)
    h = rng.uniform(-0.5, 0.5, size=(n, d.n_layers, d.d_model)).astype(np.float32)
    c = rng.uniform(-1, 1, size=(n, d.n_layers, d.hidden)).astype(np.float32)
    eout, h2, c2 = gm.run_encoder(x, h, c)
    for i in range(n):
        e0, h0, c0 = om.encoder(x[i:i + 1], h[i][:, None, :], c[i][:, None, :])
        assert np.abs(eout[i] - e0.ravel()).max() < 1e-4
        assert np.abs(h2[i] - h0[:, 0, :]).max() < 1e-4
        assert np.abs(c2[i] - c0[:, 0, :]).max() < 1e-4


def test_other_geometry_session_matches_oracle(other_model):
    from test_gpu_parity import run_oracle, run_gpu, assert_same_transcript
    pcm = speech_like_pcm(3.0, seed=1)
    want, lg0, n0 = run_oracle(other_model["om"], pcm, 1600)
    got, lg1, n1 = run_gpu(other_model["gm"], pcm, 1600)
    assert n0 == n1 and n0 > 10
    assert lg0.shape == lg1.shape and np.abs(lg0 - lg1).max() < 1e-3
    assert_same_transcript(want, got)
