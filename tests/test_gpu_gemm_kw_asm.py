"""The hand-placed K loop of GM_KW (csrc/gemm_kw_asm.inc, tools/gen_kw_asm.py) against the compiler-scheduled loop it replaces
(APRIL_KW_ASM=0): the same memory operations, the same MFMA chains and the same fold, so every output word must be the same.

  * single launches (tests/kw_asm_worker.py): rows 17 / 33 / 48 / 256, 1 .. 3 problems per launch, N = 64 and 512, both tile heights
    pinned; the projection (EPI_HR, K = 1024, kz = 8) with and without the rows' scale partials and with the activation rows behind
    a slot indirection, FFN down (EPI_RESID_SSQ, K = 2048, kz = 8) with and without the residual -- rows, state rows and the
    per-32-column sums of squares, whole buffers (what a launch must not write is part of the digest; without the partials the
    projection's output rows are undefined in every schedule and only its state rows are compared);
  * 32 sessions x 12 feeds of 100 ms on the synthetic aprilv0 model with the switch at 0 and at 1: identical callbacks (tokens,
    logits bit for bit, flags, times), no replay mismatch.

What the bits are the bits OF is pinned by tests/test_gpu_gemm_launch.py (float64 reference), which runs the default, i.e. this loop."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 120
STATE = {"dead": None}


def worker(script, args, **env):
    if STATE["dead"]:
        pytest.fail("not started: " + STATE["dead"])
    e = dict(os.environ)
    e.update({k: str(v) for k, v in env.items()})
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.join(ROOT, "tests", script)] + [str(a) for a in args],
                       env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0:
        # a signal, an abort, the time limit or a failed HIP call: no further GPU process from this module
        STATE["dead"] = "%s %r under %r ended with status %d" % (script, args, env, r.returncode)
        pytest.fail(STATE["dead"] + "\n" + r.stdout.decode()[-1500:] + "\n" + r.stderr.decode()[-1500:])
    return r.stdout.decode()


@pytest.mark.parametrize("epi,mt", [("hr", 2), ("hr", 1), ("rs", 2), ("rs", 1)])
def test_single_launches_are_bitwise_equal_between_the_loops(built, epi, mt):
    lines = {}
    for arm in (0, 1):
        out = worker("kw_asm_worker.py", [epi, mt], APRIL_KW_ASM=arm)
        assert "DONE" in out, out[-1500:]
        lines[arm] = [ln for ln in out.splitlines() if ln.startswith("CASE ")]
    want = 4 * 3 * 2 * (3 if epi == "hr" else 2)
    assert len(lines[0]) == len(lines[1]) == want
    for a, b in zip(lines[0], lines[1]):
        assert "rc=0 plan=ok written=1" in a, a
        if " hr_nossq_" in a:
            # EPI_HR without the partials: out = resid * scale + v takes its scale from an LDS word that no schedule writes in that
            # case (the engine never launches it so), so the output rows are not a function of the inputs in either loop; the state
            # rows (= v, the sums themselves) are, and must agree
            a, b = [" ".join(w for w in ln.split() if not w.startswith("out=")) for ln in (a, b)]
        assert a == b, "the two loops differ:\n%s\n%s" % (a, b)


def test_streamed_sessions_are_identical_between_the_loops(built, v0_model):
    got = {}
    for arm in (0, 1):
        out = worker("gates_tile_worker.py", [v0_model["path"], 32, 12], APRIL_KW_ASM=arm, APRIL_MAX_SESSIONS=512, APRIL_MAX_BATCH=2048)
        line = [ln for ln in out.splitlines() if ln.startswith("DIGEST")][-1].split()
        got[arm] = (line[1], int(line[2]), int(line[3]))
    assert got[0][1] > 0 and got[0][2] == 0 and got[1][2] == 0, got
    assert got[0] == got[1], "logits or callbacks differ between APRIL_KW_ASM=0 and =1"
