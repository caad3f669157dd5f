"""Worker for tests/test_gpu_gemm_kw_asm.py: single GM_KW launches (aprilx_run_gemm, as tests/gemm_launch_worker.py makes them) of
one epilogue at one pinned tile height; prints one line per case with a digest of every output word.  The parent runs it under
APRIL_KW_ASM=0 (the compiler-scheduled K loop) and =1 (the hand-placed loop of gemm_kw_asm.inc) and compares the lines.

    python tests/kw_asm_worker.py <hr|rs> <tile rows / 16>
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as R      # noqa: E402
import gemm_launch_worker as W      # noqa: E402
from gemm_ref import EPI_HR, EPI_RESID_SSQ, GM_KW, ROUTE_KW, spec      # noqa: E402

ROWS = (17, 33, 48, 256)          # a ragged last tile, one and several row tiles of either height
HIP_FAILED = W.HIP_FAILED


def cases(epi_tag, mt):
    """kz = 8 (a slab per wave, the forms the hand-placed loop exists for): the projection at K = 1024 (a fold in every stage) with and
    without the rows' scale partials and with the activation rows behind a slot indirection; FFN down at K = 2048 (a fold every other
    stage, two rounds of the ring) with and without the residual.  N = 64 and 512, 1 .. 3 problems per launch."""
    out = []
    for M in ROWS:
        for n in (1, 2, 3):
            for N in (64, 512):
                e = dict(route=ROUTE_KW, mode=GM_KW, mt=mt, fused=1)
                if epi_tag == "hr":
                    for var in ("ssq", "nossq", "aidx"):
                        s = spec(f"hr_{var}_kw{mt}_M{M}_N{N}_n{n}", "row32", EPI_HR, M, N, 1024, kz=8, n=n, force=1, kw_pin=(1, mt), expect=e)
                        s.var = var
                        out.append(s)
                else:
                    for resid in (True, False):
                        s = spec(f"rs_{'res' if resid else 'nores'}_kw{mt}_M{M}_N{N}_n{n}", "row32", EPI_RESID_SSQ, M, N, 2048, kz=8, n=n, force=1,
                                 kw_pin=(1, mt), resid=resid, expect=e)
                        s.var = ""
                        out.append(s)
    return out


def build(s):
    case = R.Case(s)
    rng = np.random.default_rng([7, abs(R.hash_name(s.name))])
    for p in case.probs:
        if s.var == "nossq":
            p.r_ssq = None
        if s.var == "aidx":                               # the rows of A live in slots: row m reads slot aidx0[m]
            p.a0 = rng.uniform(-1.0, 1.0, (s.slots, s.lda0)).astype(np.float32)
            p.aidx0 = R.injective(rng, s.M, s.slots)
    return case


def main(epi_tag, mt):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from april_asr_amd import _ffi
    lib = _ffi.lib()
    for s in cases(epi_tag, mt):
        case = build(s)
        rc, plan, bufs = W.run_case(lib, case)
        if rc == -2:                                      # a failed HIP call: nothing more on this GPU
            print(f"CASE {s.name} rc={rc}", flush=True)
            return HIP_FAILED
        ok = rc == 0 and all(plan[k] == v for k, v in s.expect.items())
        digests, nonzero = [], False
        for name in ("out", "state", "ssq"):              # whole buffers of every problem, one digest per kind
            h = hashlib.sha256()
            for b in bufs:
                if name in b:
                    h.update(np.ascontiguousarray(b[name]).tobytes())
                    nonzero = nonzero or bool(np.any(R.bits(b[name]) != 0))
            digests.append(f"{name}={h.hexdigest()[:32]}")
        print(f"CASE {s.name} rc={rc} plan={'ok' if ok else plan} written={int(nonzero)} {' '.join(digests)}", flush=True)
    print("DONE", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], int(sys.argv[2])))
