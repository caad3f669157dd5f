"""Every GEMM schedule and epilogue against a float64 reference, one launch at a time.

The other GEMM tests (test_gpu_gemm_kw.py, test_gpu_gemm_pp.py, test_gpu_gates_tile.py, test_gpu_recur_kernels.py) prove that each
schedule gives the bits of another schedule; this module is what that web hangs on: aprilx_run_gemm (csrc/gemm_debug_api.cc) runs
ONE launch the way the engine launches it, from logical A, W[K][N] and the side inputs, and tests/gemm_ref.py states what it must
compute -- the packed weight orders, every epilogue in float64, a tolerance per element, and which elements must stay unwritten.

One worker process per knob set (the knobs are read once per process), each under a time limit of its own; a worker that ends on
a signal, an abort, its time limit or a failed HIP call (a kernel's fault: the worker stops at that case and exits with a status of its
own) -- on any status but 0 -- fails every later test of the module at once, without another GPU process."""
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_launch_worker as W      # noqa: E402
from gemm_ref import GM_SLAB, GM_FULLK, GM_TILE, GM_KW, GM_PP, ROUTE_KSPLIT, ROUTE_STREAM, ROUTE_PP, ROUTE_PW, ROUTE_TILE, ROUTE_KW      # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 150
STATE = {"dead": None, "results": {}}


def run_worker(knobs):
    if STATE["dead"]:
        pytest.fail("not started: " + STATE["dead"])
    env = dict(os.environ, **W.KNOB_SETS[knobs])
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.join(ROOT, "tests", "gemm_launch_worker.py"), knobs],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out = r.stdout.decode()
    lines = [ln for ln in out.splitlines() if ln.startswith("CASE ")]
    print("\n".join(lines))
    if r.returncode != 0:
        # a signal, an abort, the time limit, a failed HIP call (W.HIP_FAILED) or anything else the worker did not end well on:
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
    bad = [r for r in results if not r["ok"]]
    worst = {}
    for r in results:
        key = (r["cls"], "binary16" if r["wt"] else "fp32")
        for buf, (ratio, _at) in r["ratios"].items():
            k2 = key + ("binary16 copies" if buf.endswith("16") else "fp32 outputs",)
            worst[k2] = max(worst.get(k2, 0.0), ratio)
    for k in sorted(worst):
        print("WORST %s %s / %s (%s): err / tol = %.3g" % ((knobs,) + k + (worst[k],)))
    assert not bad, "%d of %d cases fail:\n%s" % (len(bad), len(results), "\n".join("%s: %s" % (r["name"], r["why"]) for r in bad[:40]))


def test_the_plans_that_ran_cover_every_schedule(built):
    if STATE["dead"]:
        pytest.fail("not started: " + STATE["dead"])
    assert set(STATE["results"]) == set(W.KNOB_SETS), "a worker did not finish"
    ran = [r for rs in STATE["results"].values() for r in rs if r["rc"] == 0]
    plans = [(r["plan"], r["wt"]) for r in ran]
    has = lambda f: any(f(p, wt) for p, wt in plans)
    missing = []
    need = lambda what, f: None if has(f) else missing.append(what)
    for route in (ROUTE_KSPLIT, ROUTE_STREAM, ROUTE_PP, ROUTE_PW, ROUTE_TILE, ROUTE_KW):
        need("route %d" % route, lambda p, wt, route=route: p["route"] == route)
    for form in range(1, 7):
        need("stream form %d" % form, lambda p, wt, form=form: p["route"] == ROUTE_STREAM and p["form"] == form)
    for mt in (1, 2, 4):
        need("GM_SLAB mt %d" % mt, lambda p, wt, mt=mt: p["route"] == ROUTE_KSPLIT and p["mode"] == GM_SLAB and p["mt"] == mt)
    need("GM_FULLK", lambda p, wt: p["route"] == ROUTE_KSPLIT and p["mode"] == GM_FULLK)
    for planes in (2, 4, 8):
        need("split plan with %d planes" % planes, lambda p, wt, planes=planes: p["split"] == 1 and p["planes"] == planes)
    for mt, nt in ((4, 4), (2, 2), (1, 2)):
        need("GM_KW tile %d x %d" % (mt, nt), lambda p, wt, mt=mt, nt=nt: p["route"] == ROUTE_KW and p["mode"] == GM_KW and p["mt"] == mt and p["nt"] == nt)
    for wt in (0, 1):
        need("GM_TILE fused, wt %d" % wt, lambda p, w, wt=wt: p["route"] == ROUTE_TILE and p["mode"] == GM_TILE and p["fused"] == 1 and w == wt)
        need("GM_TILE split, wt %d" % wt, lambda p, w, wt=wt: p["route"] == ROUTE_TILE and p["mode"] == GM_TILE and p["split"] == 1 and w == wt)
    for mt in (8, 16):
        need("GM_PP mt %d" % mt, lambda p, wt, mt=mt: p["route"] == ROUTE_PP and p["mode"] == GM_PP and p["mt"] == mt)
    need("GM_TILE 128 x 128", lambda p, wt: p["route"] == ROUTE_TILE and p["mt"] == 8 and p["nt"] == 8)
    need("the 192-column form", lambda p, wt: p["route"] == ROUTE_PW and p["nt"] == 12)
    assert not missing, "no case ran on: " + ", ".join(missing)
