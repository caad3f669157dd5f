"""One plan per launch (csrc/gemm_plan.h, launch_planned in csrc/kernels_gemm.hip): whole sessions compute, bit for bit, what they
computed before the planner was restated.  tests/gemm_plan_worker.py streams the same audio through 1, 20 and 40 sessions of the
TINY and MEDIUM models, fp32 and fp16, as chunk steps and as one long feed -- launches through launch_gemm and launch_gemm_z, on
the stream kernels, GM_KW and the K-split kernels -- and its digests of every logit and callback must equal those recorded with
the same worker from the library of the commit before the change (tests/golden/gemm_plan_digests.json)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_digests.json")


def digests(paths, precision, lib=None):
    env = dict(os.environ)
    env.pop("APRIL_PRECISION", None)
    if precision == "f16":
        env["APRIL_PRECISION"] = "f16"
    if lib:
        env["APRIL_ASR_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gemm_plan_worker.py")] + paths, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    got = {}
    for line in out.splitlines():
        if line.startswith("DIGEST "):
            _, model, nsess, trace, d, chunks, mismatch = line.split()
            assert int(chunks) > 0 and int(mismatch) == 0, line
            got["%s %s %s" % (model, nsess, "traced" if trace == "1" else "graphs")] = d
    assert len(got) == 6 * len(paths), out[-3000:]
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_sessions_equal_the_parent_library_bit_for_bit(tiny_model, medium_model, precision):
    got = digests([tiny_model["path"], medium_model["path"]], precision)
    with open(GOLDEN) as f:
        want = json.load(f)[precision]
    assert got == want
