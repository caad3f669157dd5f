"""tests/gemm_ref.py checked against itself, without a GPU: the packed orders, that the chosen inputs are ones an fp32 machine stays
well inside the tolerance on (an emulation of the canonical summation order of kernels.h), and that the comparison has teeth."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as R      # noqa: E402
import gemm_launch_worker as W      # noqa: E402
from gemm_ref import EPI_PARTIAL, EPI_LSTM, EPI_BIAS_DSWISH, EPI_HR, EPI_RESID_SSQ, EPI_SLOT_STORE, AOP_TANH_ADD, spec      # noqa: E402


def test_pack_x4_round_trip():
    rng = np.random.default_rng(1)
    for K, N in ((64, 16), (128, 96), (256, 192)):
        Wm = rng.standard_normal((K, N)).astype(np.float32)
        assert np.array_equal(R.unpack_x4(R.pack_x4(Wm), K, N), Wm)


def test_pack_x32_is_the_repack_formula_applied_to_pack_x4():
    """launch_repack_x32 (kernels.h), index by index: dst[((ntile * (K / 32) + kb) * 64 + lane) * 8 + j] is the element
    W[kb * 32 + (lane >> 4) * 8 + j][ntile * 16 + (lane & 15)], read from the x4 order it is given."""
    rng = np.random.default_rng(2)
    K, N = 128, 48
    Wm = rng.standard_normal((K, N)).astype(np.float32)
    src = R.pack_x4(Wm)
    KB = K // 16
    x4 = lambda k, n: src[(((n // 16) * KB + k // 16) * 64 + ((k % 16) // 4) * 16 + n % 16) * 4 + k % 4]
    dst = np.empty(K * N, np.float32)
    for ntile in range(N // 16):
        for kb in range(K // 32):
            for lane in range(64):
                for j in range(8):
                    dst[((ntile * (K // 32) + kb) * 64 + lane) * 8 + j] = x4(kb * 32 + (lane >> 4) * 8 + j, ntile * 16 + (lane & 15))
    assert np.array_equal(dst, R.pack_x32(Wm))


def class_representatives():
    """One case per class: what the sums and the epilogue depend on, and the schedule the case is written for (route, tile rows), so
    that every form enters, the 192-column and the 128 x 128 ones included.  The emulation looks at three rows, so the case of the
    fewest rows stands for its class."""
    reps = {}
    for knobs in W.KNOB_SETS:
        for s in W.cases(knobs):
            key = (s.cls, s.epi, s.kz, s.K, s.K1, s.wt, s.tile_ok, s.waves, s.joiner, s.x_scale, s.resid, s.N if s.N <= 96 else 0,
                   s.expect.get("route"), s.expect.get("mt"), s.expect.get("nt"))
            if s.run and (key not in reps or s.M < reps[key].M):
                reps[key] = s
    return list(reps.values())


def test_fp32_emulation_of_the_canonical_order_stays_below_a_quarter_of_the_tolerance():
    """The condition that the inputs chosen are ones the reference alone stays well inside."""
    reps = class_representatives()
    assert len(reps) > 40
    worst = 0.0
    for s in reps:
        rows = min(s.M, 3)
        for p in R.Case(s).probs[:1]:
            Sx, Sh = R.sums(s, p)[:2]
            ex, eh = R.emulate32(s, p, rows)
            Sx, Sh = Sx.copy(), Sh.copy()
            Sx[:rows], Sh[:rows] = ex, eh
            ev = R.evaluate(s, p)
            emu = R.evaluate(s, p, override=(Sx, Sh))
            res = R.compare(s, p, ev, R.render(s, p, emu), rows_limit=rows)
            # (the fp32 values themselves; a binary16 copy is only in or out of its interval: the line below)
            w = max(float(np.max(np.abs(emu[k][0].astype(np.float32)[:rows] - ev[k][0][:rows]) / ev[k][1][:rows])) for k in ev)
            assert w < 0.25, (s.name, w, res)
            assert R.worst(res) <= 1.0, (s.name, res)
            worst = max(worst, w)
    print("worst emulation err / tol: %.3g over %d case classes" % (worst, len(reps)))


GATES = dict(K1=64, x_scale=True, aidx1=True)
TEETH = [
    ("drop_block", spec("gates", "t", EPI_LSTM, 17, 64, 128, **GATES)),
    ("drop_block", spec("hr", "t", EPI_HR, 17, 96, 512, kz=8)),
    ("drop_block", spec("join", "t", EPI_PARTIAL, 17, 96, 128, kz=2, a_op=AOP_TANH_ADD, joiner="ctx")),
    ("swap_k", spec("gates", "t", EPI_LSTM, 17, 64, 128, **GATES)),
    ("swap_k", spec("ffup", "t", EPI_BIAS_DSWISH, 17, 64, 64)),
    ("swap_k", spec("rs", "t", EPI_RESID_SSQ, 17, 96, 1024, kz=8)),
    ("swap_k", spec("ss", "t", EPI_SLOT_STORE, 17, 96, 64, x_scale=True, mask=True, slot=True)),
    ("swap_k", spec("ffup16", "t", EPI_BIAS_DSWISH, 33, 64, 128, wt=1, tile_ok=2, out=False, out16=True)),
    ("a1_row", spec("gates", "t", EPI_LSTM, 17, 64, 128, **GATES)),
    ("scale_both", spec("gates", "t", EPI_LSTM, 17, 64, 128, **GATES)),
    ("swap_fi", spec("gates", "t", EPI_LSTM, 17, 64, 128, **GATES)),
    ("sig_y", spec("ffup", "t", EPI_BIAS_DSWISH, 17, 64, 64)),
    ("bias_masked", spec("ss", "t", EPI_SLOT_STORE, 17, 96, 64, x_scale=True, mask=True, slot=True)),
    ("state_row", spec("hr", "t", EPI_HR, 17, 96, 128, kz=2)),
    ("state_row", spec("gates", "t", EPI_LSTM, 17, 64, 128, **GATES)),
    ("ssq_shift", spec("rs", "t", EPI_RESID_SSQ, 17, 96, 128, kz=2)),
    ("row_past_M", spec("ffup", "t", EPI_BIAS_DSWISH, 17, 64, 64)),
    ("row_past_M", spec("hr16", "t", EPI_HR, 33, 64, 256, kz=2, wt=1, tile_ok=2, out16=True, state16=True)),
    ("fp32_operands", spec("ffup16", "t", EPI_BIAS_DSWISH, 33, 64, 128, wt=1, tile_ok=2, out=False, out16=True)),
    ("fp32_operands", spec("gates_x16", "t", EPI_LSTM, 17, 64, 128, wt=1, **GATES)),
]


@pytest.mark.parametrize("mut,s", TEETH, ids=["%s-%s" % (m, s.name) for m, s in TEETH])
def test_the_comparison_rejects(mut, s):
    """one 16-k block dropped; two k rows of W swapped; A segment 1 read at `row`; the row scale on both halves; gates f and i
    exchanged; sigma(y) for sigma(y - 1); bias on masked rows; state written at `row`; the ssq granule shifted by one quad; one row
    past M written; fp32 operands where binary16 ones are stated -- each applied to the reference's own output."""
    p = R.Case(s).probs[0]
    ev = R.evaluate(s, p)
    assert R.worst(R.compare(s, p, ev, R.render(s, p, ev))) <= 1.0
    wrong = R.render(s, p, R.evaluate(s, p, mut), mut)
    res = R.compare(s, p, ev, wrong)
    assert R.worst(res) > 1.0, res


def test_swapped_k_rows_put_most_outputs_over_the_tolerance():
    s = spec("lin", "t", EPI_PARTIAL, 8, 64, 256, kz=4, a_op=AOP_TANH_ADD, joiner="aidx0")
    p = R.Case(s).probs[0]
    val, tol = R.evaluate(s, p)["planes"]
    bad = R.evaluate(s, p, "swap_k")["planes"][0]
    assert (np.abs(bad - val) > tol).mean() > 0.9


def test_no_ratio_is_a_nan():
    """0 / 0 (an exact value with no tolerance) is 0; anything else that is no finite number counts as inf, so that it cannot hide the
    buffer's worst ratio from a comparison or an argmax."""
    nan, inf = np.nan, np.inf
    r = R.err_ratio(np.array([0.0, 1.0, nan, inf, 1.0, 0.5]), np.array([0.0, 0.0, 1.0, 1.0, nan, 1.0]))
    assert r.tolist() == [0.0, inf, inf, inf, inf, 0.5]
    s = spec("nan", "t", EPI_BIAS_DSWISH, 17, 64, 64)
    p = R.Case(s).probs[0]
    ev = R.evaluate(s, p)
    bufs = R.render(s, p, ev)
    ev["out"][1][0, 0] = 0.0                              # no tolerance at an element that is not exact: fp32 of a float64 value
    bufs["out"][3, 5] = np.inf
    assert R.compare(s, p, ev, bufs)["out"][0] == inf


def test_a_failed_hip_call_ends_the_worker_and_every_later_gpu_process(monkeypatch, capsys):
    """aprilx_run_gemm returns -2 when a HIP call fails, a kernel's fault among them: the worker runs no further case and exits with
    HIP_FAILED; the parent then fails every later test of the module without starting a process.  (No GPU: a library that only
    answers -2, and a subprocess.run that only hands that status back.)"""
    import subprocess
    import test_gpu_gemm_launch as T

    class Lib:
        calls = 0

        def aprilx_run_gemm(self, *a):
            Lib.calls += 1
            return -2

    assert W.main("nofullk", Lib()) == W.HIP_FAILED and Lib.calls == 1
    out = capsys.readouterr().out
    assert out.count("CASE ") == 1 and "RESULT " in out

    started = []

    def run(cmd, **kw):
        started.append(cmd)
        return subprocess.CompletedProcess(cmd, W.HIP_FAILED, stdout=out.encode(), stderr=b"")

    monkeypatch.setattr(T.subprocess, "run", run)
    monkeypatch.setattr(T, "STATE", {"dead": None, "results": {}})
    with pytest.raises(pytest.fail.Exception, match="status %d" % W.HIP_FAILED):
        T.run_worker("default")
    assert len(started) == 1 and T.STATE["dead"]
    with pytest.raises(pytest.fail.Exception, match="not started"):
        T.run_worker("norecur")
    with pytest.raises(pytest.fail.Exception, match="not started"):
        T.test_the_plans_that_ran_cover_every_schedule(None)
    assert len(started) == 1


def test_nothing_is_written_when_the_launch_sits_out():
    s = spec("off", "t", EPI_HR, 17, 96, 128, kz=2, run=False)
    p = R.Case(s).probs[0]
    ev = R.evaluate(s, p)
    blank = R.render(s, p, ev)
    assert all(np.all(R.bits(b) == R.bits(R.pattern(b.shape, b.dtype))) for b in blank.values())
    assert R.worst(R.compare(s, p, ev, blank)) == 0.0
    s_on = spec("off", "t", EPI_HR, 17, 96, 128, kz=2)
    assert R.worst(R.compare(s, p, ev, R.render(s_on, p, ev))) == np.inf
