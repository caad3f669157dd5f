"""The GEMM planner (csrc/gemm_plan.h) against the decision table recorded from the planner it replaced
(tests/golden/gemm_plan_table.npz; its `header` array names the commit and the grid).

1. tests/cpp/gemm_plan_test.cc, compiled with g++ from the header alone under AddressSanitizer + UBSan: plan_gemm and its parts
   reproduce every recorded row exactly -- default knobs over the whole grid, every knob value and bench-tool pin over the two
   large models, knobs passed as values in one process -- and the engine's question agrees with the launch on every row-epilogue row.
2. Through the built library (no GPU): gemm_plan(const GemmArgs &) finds the capabilities the kernel files' predicates gave when the
   table was recorded, and its answer is the table's, for rows spread over all routes."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "april_asr_amd", "csrc")
TABLE = os.path.join(ROOT, "tests", "golden", "gemm_plan_table.npz")
EPI_PARTIAL, EPI_HR, EPI_RESID_SSQ, EPI_SLOT_STORE = 0, 3, 4, 5
GM_FULLK, GM_TILE, GM_KW, GM_PP = 1, 2, 3, 4


def load_table():
    z = np.load(TABLE)
    t = {k: z[k] for k in z.files}
    t["query"] = np.ascontiguousarray(t.pop("query_t").T).astype(np.int32)
    t["default_out"] = np.ascontiguousarray(t.pop("default_out_t").T).astype(np.int32)
    t["diff_out"] = np.ascontiguousarray(t.pop("diff_out_t").T).astype(np.int32)
    step = t.pop("diff_query_step").astype(np.int64)
    dset = t["diff_setting"].astype(np.int64)
    # the row index of a diff entry: steps summed inside its setting
    total = np.cumsum(step)
    first = np.flatnonzero(np.diff(dset, prepend=-1) != 0)
    before = np.concatenate([[0], total[first[1:] - 1]])
    t["diff_query"] = (total - np.repeat(before, np.diff(np.append(first, len(step))))).astype(np.int32)
    return t


def test_plan_gemm_reproduces_the_recorded_table_under_asan_ubsan(tmp_path):
    t = load_table()
    n, ns, nd = len(t["query"]), len(t["settings"]), len(t["diff_query"])
    assert n > 50000 and ns == 37 and t["query"].shape[1] == 26 and t["default_out"].shape == (n, 9) and t["settings"].shape[1] == 18
    assert t["diff_query"].min() >= 0 and t["diff_query"].max() < n and (t["subset"][t["diff_query"]] == 1).all()
    flat = str(tmp_path / "gemm_plan_table.bin")
    with open(flat, "wb") as f:
        np.array([n, ns, nd], dtype=np.int32).tofile(f)
        for a in (t["query"], t["default_out"], t["subset"], t["settings"], t["diff_setting"], t["diff_query"], t["diff_out"]):
            np.ascontiguousarray(a, dtype=np.int32).tofile(f)
    exe = str(tmp_path / "gemm_plan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "gemm_plan_test.cc"), "-o", exe], timeout=600)
    r = subprocess.run([exe, flat], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0 and "all checks passed" in out, out[-4000:]


def test_gemm_plan_of_an_argument_block_fills_the_recorded_capabilities():
    from april_asr_amd import _ffi
    lib = _ffi.lib()
    t = load_table()
    q, o = t["query"], t["default_out"]
    row_epi = np.isin(q[:, 6], (EPI_HR, EPI_RESID_SSQ, EPI_SLOT_STORE))
    stream = (q[:, 22] != 0) & (o[:, 0] == 0)
    ok = o[:, 1] == 0
    picks = []
    rng = np.random.default_rng(5)
    # rows of every route (stream kernels by form, GM_PP 128 / 192 columns, GM_TILE, GM_KW, K-split slab / full K), split row epilogues, errors
    classes = [stream & (q[:, 22] == form) for form in range(1, 7)] + \
              [ok & ~stream & (o[:, 5] == GM_PP) & (o[:, 3] == 8), ok & ~stream & (o[:, 5] == GM_PP) & (o[:, 3] == 12), ok & ~stream & (o[:, 5] == GM_TILE),
               ok & ~stream & (o[:, 5] == GM_KW), ok & ~stream & (o[:, 5] == 0), ok & ~stream & (o[:, 5] == GM_FULLK), row_epi & (o[:, 6] == 0) & (o[:, 7] > 1),
               o[:, 1] == 1, o[:, 1] == 3, (q[:, 23] != 0) & (o[:, 0] == 1), q[:, 25] != 0]
    for c in classes:
        idx = np.flatnonzero(c)
        assert idx.size > 0
        picks += list(rng.choice(idx, size=min(4, idx.size), replace=False))
    assert len(picks) >= 48
    for i in picks:
        inp = np.ascontiguousarray(q[i, :22], dtype=np.int32)
        out = np.zeros(13, dtype=np.int32)
        assert lib.aprilx_gemm_plan_debug(inp.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 0
        caps, (route, form, mode, mt, nt, zs, planes, fused, error) = out[:4], out[4:]
        assert list(caps) == list(q[i, 22:26]), (i, list(q[i]), list(out))
        if row_epi[i] and o[i, 6] == 0:          # the question's answer: not fused, the partial form's planes
            assert (fused, planes, error) == (0, o[i, 7], 0), (i, list(q[i]), list(out), list(o[i]))
            continue
        assert error == o[i, 1], (i, list(q[i]), list(out), list(o[i]))
        assert (route == 1) == bool(stream[i]) and (route != 1 or form == q[i, 22]), (i, list(q[i]), list(out), list(o[i]))
        if error == 0:
            assert (mt, nt, zs, mode) == tuple(o[i, 2:6]), (i, list(q[i]), list(out), list(o[i]))
