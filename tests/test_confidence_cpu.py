"""Per-token confidences, the parts that need no GPU: the ABI (AprilxTokenInfo, the grown AprilxStats, the
three entry points), the unchanged host-only search (tokens keep reserved == NULL), and the float64 statement of the contract that
tests/test_gpu_confidence.py holds the device to -- checked here on its own, together with the claim that the contract's error
bound is one the contract alone satisfies (an fp32 emulation of a legal summation order stays inside it)."""
import ctypes as C
import os
import subprocess

import numpy as np

import confidence_ref as R
from april_asr_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFO_FIELDS = ("size", "n_alt", "eval_index", "lse", "token_logprob", "blank_logprob", "reserved0", "alt_id", "alt_logit")


def test_token_info_and_stats_layout_equal_the_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "aprilx_engine.h"\nint main(void){'
                   'printf("%zu ", sizeof(AprilxTokenInfo));'
                   + "".join('printf("%%zu ", offsetof(AprilxTokenInfo, %s));' % f for f in INFO_FIELDS)
                   + 'printf("%zu %zu %zu", sizeof(AprilxStats), offsetof(AprilxStats, resample_launches), offsetof(AprilxStats, confidence_records));'
                   'return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    T = _ffi.AprilxTokenInfo
    assert out[0] == C.sizeof(T) == 96
    assert out[1:1 + len(INFO_FIELDS)] == [getattr(T, f).offset for f in INFO_FIELDS] == [0, 4, 8, 16, 20, 24, 28, 32, 64]
    S = _ffi.AprilxStats
    assert out[-3:] == [C.sizeof(S), S.resample_launches.offset, S.confidence_records.offset]
    assert S.confidence_records.offset + 8 == C.sizeof(S), "confidence_records is the last field: the struct grows at its end"


def test_entry_points_are_exported(built):
    L = _ffi.lib()
    names = ("aprilx_session_set_confidence", "aprilx_session_confidence", "aprilx_run_confidence")
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.LIB_PATH]).decode()
    defined = {l.split()[-1] for l in out.splitlines() if len(l.split()) >= 3}
    for n in names:
        assert n in _ffi.EXPORTED_ENGINE_SYMBOLS and hasattr(L, n) and n in defined, n
    assert L.aprilx_session_set_confidence(None, 4) == -1 and L.aprilx_session_confidence(None) == 0
    assert L.aprilx_run_confidence(None, 1, None, 4, None) == -1


def test_host_only_search_keeps_reserved_null(tiny_model):
    """aprilx_model_load_host + aprilx_greedy_*: nothing changes, every token of every result carries reserved == NULL"""
    import april_asr_amd as A
    m = A.Model.load_host_only(tiny_model["path"])
    L = m._L
    seen = []

    def on_result(_ud, rtype, count, toks):
        seen.append((int(rtype), [(toks[i].token, float(toks[i].logprob), toks[i].reserved) for i in range(count)]))

    cb = _ffi.HANDLER(on_result)
    g = L.aprilx_greedy_create(m._handle, cb, None)
    assert g
    ctx = (C.c_int32 * 2)()
    now = 0
    for idx, mx, bl in [(3, 5.0, 1.0), (4, 2.0, 3.0), (5, 6.0, 0.0), (6, 1.0, 2.5), (7, 4.0, -1.0)]:
        now += 160
        L.aprilx_greedy_step(g, idx, mx, bl, 1.0, now, ctx)
    L.aprilx_greedy_step(g, 9, -5.0, 9.0, 1.0, now + 5000, ctx)          # silence: FINAL
    L.aprilx_greedy_finish(g)
    L.aprilx_greedy_free(g)
    tokens = [t for _, toks in seen for t in toks]
    assert len(tokens) >= 6 and any(t == 2 for t, _ in seen) and any(lp < 0 for _, lp, _ in tokens)
    assert all(r is None for _, _, r in tokens)
    L.aam_free(m._handle); m._handle = None


def test_reference_ties_and_short_rows():
    row = np.array([9.0, 1.0, 3.0, 3.0, -2.0, 3.0, 0.5], np.float32)       # blank 0 holds the maximum; 2, 3, 5 tie
    lse, ids, lg, bl = R.reference(row, 0, 4)
    assert list(ids) == [2, 3, 5, 1] and list(lg) == [3.0, 3.0, 3.0, 1.0]
    want = np.log(np.exp(row.astype(np.float64)).sum())
    assert abs(lse - want) < 1e-12 and abs(bl - (9.0 - want)) < 1e-12
    assert list(R.reference(row, 0, 2)[1]) == [2, 3]                      # the tie crosses the K boundary: lower ids stay
    assert list(R.reference(row, 0, 8)[1]) == [2, 3, 5, 1, 6, 4]          # K larger than the number of candidates: V - 1 entries
    assert list(R.reference(row, 2, 3)[1]) == [0, 3, 5]                   # another blank id


def test_reference_equal_row_and_nan_row():
    for v, val in ((40, 1.5), (500, -7.25), (1100, 300.0)):
        lse, ids, lg, bl = R.reference(np.full(v, val, np.float32), 0, 8)
        assert abs(lse - (val + np.log(v))) < 1e-9 and list(ids) == list(range(1, 9)) and abs(bl + np.log(v)) < 1e-9
    lse, ids, lg, bl = R.reference(np.full(40, np.nan, np.float32), 0, 4)
    assert np.isnan(lse) and ids.size == 0 and lg.size == 0
    row = np.full(40, -1e30, np.float32); row[0] = 2.0                   # nothing beats the initial value except the blank
    assert R.reference(row, 0, 4)[1].size == 0


def test_fp32_emulation_of_a_legal_order_stays_inside_the_bound():
    """256 strided partial sums + butterfly in fp32 with numpy's float32 exp / log against float64 on the same fp32 logits: the
    bound of DESIGN.md section 12 holds with room to spare on 10 000 random rows per (V, scale), row offsets up to +-300."""
    rng = np.random.default_rng(20240612)
    worst = 0.0
    for vocab in (40, 500, 1100):
        for scale in (1.0, 10.0, 100.0):
            for _ in range(5):
                rows = R.random_rows(rng, 2000, vocab, scale)
                got = R.lse_fp32_emulation(rows).astype(np.float64)
                v = rows.astype(np.float64)
                m = v.max(axis=1)
                lse64 = m + np.log(np.exp(v - m[:, None]).sum(axis=1))
                ratio = np.abs(got - lse64) / (3e-6 + 2.0 ** -23 * np.abs(lse64))
                assert ratio.max() <= 1.0, (vocab, scale, ratio.max())
                # a log-softmax formed from it in fp32 (v - lse, one more rounding), for the row's first entries
                ls32 = (rows[:, :8] - got.astype(np.float32)[:, None]).astype(np.float32).astype(np.float64)
                ls64 = v[:, :8] - lse64[:, None]
                r2 = np.abs(ls32 - ls64) / (3e-6 + 2.0 ** -23 * (np.abs(lse64)[:, None] + np.abs(ls64)))
                assert r2.max() <= 1.0, (vocab, scale, r2.max())
                worst = max(worst, float(ratio.max()), float(r2.max()))
    print("fp32 emulation: worst error = %.3f of the bound" % worst)
