"""One process per knob set: runs a list of single GEMM launches (aprilx_run_gemm) and compares each with tests/gemm_ref.py.

    python tests/gemm_launch_worker.py <knob set>        (the parent sets the knob set's environment)

Prints one line per case -- the plan that ran and the worst err / tol per buffer -- and a last line RESULT <json>.  After a failed
HIP call (aprilx_run_gemm returns -2: a kernel's fault shows up there) it runs no further case and exits with status HIP_FAILED.  The case
lists are stated here once; tests/test_gemm_ref_cpu.py walks the same lists without a GPU.  Shapes are the smallest each kernel
admits (the capability predicates beside the kernels): K = 64 kz for the K-split kernels, 512 (kz 2) / 1024 (kz 8) for GM_KW,
128 / 256 for GM_PP and its halves, 256 for the 192-column form; rows around every tile height of the form under test.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as R      # noqa: E402
from gemm_ref import (EPI_PARTIAL, EPI_LSTM, EPI_BIAS_DSWISH, EPI_HR, EPI_RESID_SSQ, EPI_SLOT_STORE, EPI_XPART, AOP_TANH_ADD,      # noqa: E402
                      GM_SLAB, GM_FULLK, GM_TILE, GM_KW, GM_PP, ROUTE_KSPLIT, ROUTE_STREAM, ROUTE_PP, ROUTE_PW, ROUTE_TILE, ROUTE_KW, spec)

KNOB_SETS = {"default": {}, "norecur": {"APRIL_RECUR_KERNELS": "0"}, "nofullk": {"APRIL_FULLK": "0"}}
PLAN_KEYS = ("recur", "kw", "pp", "pw", "route", "form", "mode", "mt", "nt", "zs", "planes", "fused", "error", "split")
# stream-kernel forms (aprilx_stream_form in include/aprilx_engine.h)
F_GATES_H, F_HR, F_GATES, F_XPART, F_DSWISH, F_RESID = 1, 2, 3, 4, 5, 6
HIP_FAILED = 3            # the worker's exit status after a failed HIP call: the parent starts no further GPU process
KSPLIT_MT = lambda M: 1 if M <= 16 else 2 if M <= 32 else 4      # the K-split kernels' slab tiles by rows (gemm_plan.h)


def around(tile):
    return [tile - 1, tile, tile + 1, 2 * tile + 3]


def halves(name, cls, M, N, K, expect_all, expect_x, expect_h, **kw):
    """The gates GEMM in one launch and as its layer-major halves: three linked cases that share their inputs; the worker feeds
    the X half's output to the H half as p_add and compares H with the one-launch form bit for bit."""
    a = spec(name + "_all", cls, EPI_LSTM, M, N, K, K1=K // 2, x_scale=True, aidx1=True, expect=expect_all, **kw)
    x = spec(name + "_x", cls, EPI_XPART, M, N, K, K1=K // 2, x_scale=True, waves=0x3, expect=expect_x, **dict(kw, out=True, out16=False))
    h = spec(name + "_h", cls, EPI_LSTM, M, N, K, K1=K // 2, aidx1=True, p_add=True, waves=0xC, expect=expect_h, **kw)
    x.link, h.link, a.link = ("x", a.name), ("h", a.name), None
    return [a, x, h]


def cases(knobs):
    out = []
    add = out.append
    stream = knobs != "norecur"
    ks = lambda M, **e: dict(route=ROUTE_KSPLIT, mode=GM_SLAB, mt=KSPLIT_MT(M), **e)
    if knobs in ("default", "norecur"):
        rows = [1, 15, 16] if knobs == "norecur" else [1, 15, 16, 17, 31, 32, 33, 35, 63, 64, 65, 131]
        # ---- class 1: fp32 slab epilogues on the K-split kernels and the stream forms
        for M in rows:
            st = stream and M <= 16
            for N in (64, 192):
                add(spec(f"gates_M{M}_N{N}", "slab32", EPI_LSTM, M, N, 128, K1=64, x_scale=True, aidx1=True,
                         expect=dict(route=ROUTE_STREAM, form=F_GATES) if st else ks(M)))
                add(spec(f"ffup_M{M}_N{N}", "slab32", EPI_BIAS_DSWISH, M, N, 64, expect=dict(route=ROUTE_STREAM, form=F_DSWISH) if st else ks(M)))
            add(spec(f"conv3_M{M}", "slab32", EPI_BIAS_DSWISH, M, 16, 64, expect=dict(route=ROUTE_STREAM, form=F_DSWISH) if st else ks(M)))
        for M in ([1, 16] if knobs == "norecur" else [1, 16, 17, 35, 67]):
            st = stream and M <= 16
            out.extend(halves(f"halves_M{M}", "slab32", M, 64, 128,
                              dict(route=ROUTE_STREAM, form=F_GATES) if st else ks(M), dict(route=ROUTE_STREAM, form=F_XPART) if st else ks(M),
                              dict(route=ROUTE_STREAM, form=F_GATES_H) if st else ks(M)))
        # ---- class 2: fp32 row epilogues, fused with all of K in the workgroup (force_fullk)
        for epi, tag, form, kw in ((EPI_HR, "hr", F_HR, {}), (EPI_RESID_SSQ, "rs", F_RESID, {}), (EPI_RESID_SSQ, "rs0", F_RESID, dict(resid=False)),
                                   (EPI_SLOT_STORE, "ss", 0, dict(x_scale=True, mask=True, slot=True)), (EPI_SLOT_STORE, "ss0", 0, {})):
            for kz in (1, 2, 4, 8):
                for M in ([1, 15, 16] if knobs == "norecur" else [1, 15, 16, 17, 35]):
                    for N in ((32, 96, 192) if M in (1, 17) else (96,)):
                        e = dict(route=ROUTE_KSPLIT, mode=GM_FULLK if kz >= 4 else GM_SLAB, fused=1, split=0)
                        if stream and M <= 16 and form:
                            e = dict(route=ROUTE_STREAM, form=form, fused=1, split=0)
                        add(spec(f"{tag}_fused_kz{kz}_M{M}_N{N}", "row32", epi, M, N, 64 * kz, kz=kz, force=1, expect=e, **kw))
    if knobs == "default":
        # ---- class 2: split planes + row kernel at planes 1, 2, 4, 8 (GM_SLAB at mt 1, 2, 4)
        for epi, tag, kw in ((EPI_HR, "hr", {}), (EPI_RESID_SSQ, "rs", {}), (EPI_SLOT_STORE, "ss", dict(x_scale=True, mask=True, slot=True))):
            for kz in (1, 2, 4, 8):
                for M in (1, 15, 16, 17, 31, 32, 33, 35, 63, 64, 65, 131):
                    N = 96 if M != 17 else 192
                    add(spec(f"{tag}_split_kz{kz}_M{M}", "row32", epi, M, N, 64 * kz, kz=kz,
                             expect=dict(route=ROUTE_KSPLIT, mode=GM_SLAB, mt=KSPLIT_MT(M), planes=kz, fused=0, split=1), **kw))
        add(spec("rs_split_k2_kz4_M35", "row32", EPI_RESID_SSQ, 35, 96, 512, kz=4, expect=dict(route=ROUTE_KSPLIT, planes=4, split=1)))
        # GM_KW on each of its tiles, pinned: K = 512 at kz 2, 1024 at kz 8 (its two-stage ring once round), and a second round
        for mt, N in ((4, 64), (4, 192), (2, 96), (1, 96)):
            for M in [m for m in around(16 * mt) if m >= 3]:
                for epi, tag in ((EPI_HR, "hr"), (EPI_RESID_SSQ, "rs")):
                    if epi == EPI_HR and M <= 16:
                        continue                          # (the projection's stream kernel keeps <= 16 rows: gemm_plan.h kw_before_recur)
                    for kz, K in ((2, 512), (8, 1024)) + (((2, 1024),) if M == 16 * mt + 1 else ()):
                        add(spec(f"{tag}_kw{mt}_kz{kz}_K{K}_M{M}_N{N}", "row32", epi, M, N, K, kz=kz, force=1, kw_pin=(1, mt),
                                 expect=dict(route=ROUTE_KW, mode=GM_KW, mt=mt, fused=1)))
        # GM_TILE by pin: mt 2 / 4 fused (all of K) and with zs < kz (planes + row kernel).  Rows from 32: the planner gives an fp32
        # (tile_ok 1) GEMM of fewer rows no GM_TILE plan, pinned or not (plan_tile in gemm_plan.h: M < min_rows), so M = 1 and
        # tile - 1 = 31 of the 32-row tile cannot be reached; the binary16 forms below (tile_ok 2) run at every row count and take them
        for mt in (2, 4):
            for M in ([32, 33, 67] if mt == 2 else [63, 64, 65, 131]):
                for epi, tag, kw in ((EPI_HR, "hr", {}), (EPI_RESID_SSQ, "rs", {}), (EPI_SLOT_STORE, "ss", dict(x_scale=True, mask=True, slot=True))):
                    for kz in (1, 2, 4):
                        N = 192 if kz == 2 else 64
                        add(spec(f"{tag}_tile{mt}_fused_kz{kz}_M{M}", "row32", epi, M, N, 64 * kz, kz=kz, tile_ok=1, force=1, tile_pin=(1, mt, 0),
                                 expect=dict(route=ROUTE_TILE, mode=GM_TILE, mt=mt, fused=1, split=0), **kw))
                        if kz > 1:
                            add(spec(f"{tag}_tile{mt}_split_kz{kz}_M{M}", "row32", epi, M, N, 64 * kz, kz=kz, tile_ok=1, tile_pin=(1, mt, 1),
                                     expect=dict(route=ROUTE_TILE, mode=GM_TILE, mt=mt, zs=1, planes=kz, fused=0, split=1), **kw))
        # ---- class 3: the joiner
        for mode in ("aidx0", "aidx0b", "ctx"):
            for M in (1, 17, 35):
                for kz, N in ((1, 96), (2, 48), (4, 96)):
                    add(spec(f"join_{mode}_kz{kz}_M{M}_N{N}", "joiner", EPI_PARTIAL, M, N, 64 * kz, kz=kz, a_op=AOP_TANH_ADD, joiner=mode,
                             expect=dict(route=ROUTE_KSPLIT, mode=GM_SLAB, planes=kz)))
            add(spec(f"join_{mode}_fullk", "joiner", EPI_PARTIAL, 17, 96, 256, kz=4, a_op=AOP_TANH_ADD, joiner=mode, force=1,
                     expect=dict(route=ROUTE_KSPLIT, mode=GM_FULLK, planes=1)))
        # ---- class 4: binary16 operands.  The x16 K-split form (tile_ok 0) ...
        for M in (1, 17, 35, 67):
            add(spec(f"x16_ffup_M{M}", "f16", EPI_BIAS_DSWISH, M, 64, 64, wt=1, expect=ks(M)))
            add(spec(f"x16_gates_M{M}", "f16", EPI_LSTM, M, 64, 128, K1=64, x_scale=True, aidx1=True, wt=1, expect=ks(M)))
            add(spec(f"x16_hr_M{M}", "f16", EPI_HR, M, 96, 128, kz=2, wt=1, force=1, expect=dict(route=ROUTE_KSPLIT, fused=1)))
            add(spec(f"x16_rs_split_M{M}", "f16", EPI_RESID_SSQ, M, 96, 256, kz=4, wt=1, expect=dict(route=ROUTE_KSPLIT, planes=4, split=1)))
        # ... and the tile engines' forms (tile_ok 2): GM_TILE on 32 / 64-row tiles (a chunk is whole 32-k blocks: K = 128 kz at the least),
        t16 = dict(wt=1, tile_ok=2)
        for M in (1, 31, 32, 33, 67):
            add(spec(f"t16_ffup_M{M}", "f16", EPI_BIAS_DSWISH, M, 64, 128, out=False, out16=True, expect=dict(route=ROUTE_TILE, mt=2, fused=1), **t16))
            out.extend(halves(f"t16_halves_M{M}", "f16", M, 64, 128, *(dict(route=ROUTE_TILE, mt=2),) * 3, out=False, out16=True, **t16))
            for kz in (1, 2):
                add(spec(f"t16_hr_fused_kz{kz}_M{M}", "f16", EPI_HR, M, 64, 128 * kz, kz=kz, force=1, out16=True, state16=True,
                         expect=dict(route=ROUTE_TILE, mt=2, fused=1, split=0), **t16))
                add(spec(f"t16_rs_fused_kz{kz}_M{M}", "f16", EPI_RESID_SSQ, M, 192, 128 * kz, kz=kz, force=1, out16=True,
                         expect=dict(route=ROUTE_TILE, mt=2, fused=1, split=0), **t16))
            add(spec(f"t16_hr_split_M{M}", "f16", EPI_HR, M, 64, 512, kz=4, out16=True, state16=True, expect=dict(route=ROUTE_TILE, fused=0, split=1), **t16))
            add(spec(f"t16_rs_split_M{M}", "f16", EPI_RESID_SSQ, M, 64, 256, kz=2, out16=True, expect=dict(route=ROUTE_TILE, fused=0, split=1), **t16))
        for M in (63, 64, 65, 131):
            add(spec(f"t16_rs_tile4_M{M}", "f16", EPI_RESID_SSQ, M, 64, 256, kz=2, force=1, out16=True, tile_pin=(-1, 4, 0),
                     expect=dict(route=ROUTE_TILE, mt=4, fused=1), **t16))
            add(spec(f"t16_ffup_tile4_M{M}", "f16", EPI_BIAS_DSWISH, M, 64, 128, out=False, out16=True, tile_pin=(-1, 4, 0), expect=dict(route=ROUTE_TILE, mt=4), **t16))
        # 128 x 128 GM_TILE tiles: from 192 of them per launch (three problems of 8 x 8 tiles), GM_PP off
        for M in (1021, 1024, 1025):
            add(spec(f"t16_ffup_big_M{M}", "f16", EPI_BIAS_DSWISH, M, 1024, 128, n=3, out=False, out16=True, pp_pin=(0, 0), expect=dict(route=ROUTE_TILE, mt=8, nt=8), **t16))
        # GM_PP at 128 and 256 rows (pinned), both halves; the 256 x 192 form
        for mt in (8, 16):
            for M in [1] + around(16 * mt):
                e = dict(route=ROUTE_PP, mode=GM_PP, mt=mt)
                add(spec(f"pp{mt}_ffup_M{M}", "f16", EPI_BIAS_DSWISH, M, 384 if M == 16 * mt + 1 else 128, 128, out=False, out16=True, pp_pin=(1, mt), expect=e, **t16))
                out.extend(halves(f"pp{mt}_halves_M{M}", "f16", M, 128, 256, e, e, e, out=False, out16=True, pp_pin=(1, mt), **t16))
            add(spec(f"pp{mt}_ffup_k2", "f16", EPI_BIAS_DSWISH, 16 * mt + 1, 128, 384, out=False, out16=True, pp_pin=(1, mt), expect=dict(route=ROUTE_PP, mt=mt), **t16))
        # (the planner reaches it through plan_pp, whose tiles are 128 columns: N a multiple of 384)
        for M in [1] + around(256):
            e = dict(route=ROUTE_PW, mode=GM_PP, nt=12)
            add(spec(f"pw_ffup_M{M}", "f16", EPI_BIAS_DSWISH, M, 768 if M == 257 else 384, 256, out=False, out16=True, pp_pin=(1, 12), expect=e, **t16))
            add(spec(f"pw_gates_M{M}", "f16", EPI_LSTM, M, 384, 256, K1=128, x_scale=True, aidx1=True, out=False, out16=True, pp_pin=(1, 12), expect=e, **t16))
        add(spec("pw_ffup_k2", "f16", EPI_BIAS_DSWISH, 257, 384, 512, out=False, out16=True, pp_pin=(1, 12), expect=dict(route=ROUTE_PW), **t16))
        # ---- row scales of more partials than a thread's stage registers hold (rows_scale_park in epilogue.h fetches them through its
        # `load` behind the K loop): TPR = threads / tile rows threads share a row and stage 4 partials each (16 on GM_PP), so a 64-row
        # tile of four waves needs more than 16 groups and the 256-row GM_PP tile of eight waves more than 32.  (The 192-column form
        # admits 27 groups at the most and always stages; GM_KW's 16-row and 64 x 64 tiles never stage: the hr_kw1 / hr_kw4 cases.)
        big_x = dict(K1=576, x_scale=True, aidx1=True)            # x_scale.groups = 576 / 32 = 18
        add(spec("gates_xg18_M35", "slab32", EPI_LSTM, 35, 64, 1152, expect=ks(35), **big_x))
        add(spec("x16_gates_xg18_M35", "f16", EPI_LSTM, 35, 64, 1152, wt=1, expect=ks(35), **big_x))
        add(spec("hr_tile4_rg18_M65", "row32", EPI_HR, 65, 576, 64, tile_ok=1, force=1, tile_pin=(1, 4, 0),      # r_scale.groups = 576 / 32 = 18
                 expect=dict(route=ROUTE_TILE, mode=GM_TILE, mt=4, fused=1, split=0)))
        add(spec("t16_gates_tile4_xg18_M65", "f16", EPI_LSTM, 65, 64, 1152, out=False, out16=True, tile_pin=(-1, 4, 0),
                 expect=dict(route=ROUTE_TILE, mt=4), **big_x, **t16))
        add(spec("pp16_gates_xg34_M257", "f16", EPI_LSTM, 257, 128, 2176, K1=1088, x_scale=True, aidx1=True, out=False, out16=True, pp_pin=(1, 16),
                 expect=dict(route=ROUTE_PP, mode=GM_PP, mt=16), **t16))      # x_scale.groups = 1088 / 32 = 34
        # ---- z-batched launches: n = 2 and 3 problems with pointers of their own
        add(spec("z2_gates_M67", "z", EPI_LSTM, 67, 64, 128, n=2, K1=64, x_scale=True, aidx1=True, expect=ks(67)))
        add(spec("z3_ffup_M35", "z", EPI_BIAS_DSWISH, 35, 192, 64, n=3, expect=ks(35)))
        add(spec("z2_gates_stream_M4", "z", EPI_LSTM, 4, 64, 128, n=2, K1=64, x_scale=True, aidx1=True, expect=dict(route=ROUTE_STREAM, form=F_GATES)))
        add(spec("z3_hr_stream_M4", "z", EPI_HR, 4, 96, 128, n=3, kz=2, force=1, expect=dict(route=ROUTE_STREAM, form=F_HR)))
        add(spec("z2_hr_fullk_M35", "z", EPI_HR, 35, 96, 256, n=2, kz=4, force=1, expect=dict(route=ROUTE_KSPLIT, mode=GM_FULLK, fused=1)))
        add(spec("z3_rs_slab_M35", "z", EPI_RESID_SSQ, 35, 96, 128, n=3, kz=2, force=1, expect=dict(route=ROUTE_KSPLIT, mode=GM_SLAB, fused=1)))
        add(spec("z2_rs_kw_M35", "z", EPI_RESID_SSQ, 35, 96, 512, n=2, kz=2, force=1, kw_pin=(1, 2), expect=dict(route=ROUTE_KW, mt=2)))
        add(spec("z3_hr_tile_split_M67", "z", EPI_HR, 67, 64, 256, n=3, kz=4, tile_ok=1, tile_pin=(1, 2, 1), expect=dict(route=ROUTE_TILE, planes=4, split=1)))
        add(spec("z2_pp_gates_M129", "z", EPI_LSTM, 129, 128, 256, n=2, K1=128, x_scale=True, aidx1=True, out=False, out16=True, pp_pin=(1, 8), expect=dict(route=ROUTE_PP, mt=8), **t16))
        add(spec("z3_t16_hr_M33", "z", EPI_HR, 33, 64, 256, n=3, kz=2, force=1, out16=True, state16=True, expect=dict(route=ROUTE_TILE, fused=1), **t16))
        # ---- class 5: run_flag != run_gen, one case of each route: nothing written
        add(spec("off_ksplit", "runflag", EPI_BIAS_DSWISH, 17, 64, 64, run=False, expect=ks(17)))
        add(spec("off_stream", "runflag", EPI_LSTM, 4, 64, 128, K1=64, x_scale=True, aidx1=True, run=False, expect=dict(route=ROUTE_STREAM)))
        add(spec("off_rows", "runflag", EPI_HR, 17, 96, 128, kz=2, run=False, expect=dict(route=ROUTE_KSPLIT, split=1)))
        add(spec("off_kw", "runflag", EPI_HR, 33, 96, 512, kz=2, force=1, kw_pin=(1, 2), run=False, expect=dict(route=ROUTE_KW)))
        add(spec("off_tile", "runflag", EPI_RESID_SSQ, 33, 64, 64, tile_ok=1, force=1, tile_pin=(1, 2, 0), run=False, expect=dict(route=ROUTE_TILE)))
        add(spec("off_pp", "runflag", EPI_BIAS_DSWISH, 129, 128, 128, out=False, out16=True, pp_pin=(1, 8), run=False, expect=dict(route=ROUTE_PP), **t16))
        add(spec("off_pw", "runflag", EPI_BIAS_DSWISH, 257, 384, 256, out=False, out16=True, pp_pin=(1, 12), run=False, expect=dict(route=ROUTE_PW), **t16))
    if knobs == "nofullk":
        # APRIL_FULLK=0: no fused row epilogue on the K-split kernels, whatever the caller asks: planes + row kernel
        for epi, tag, kw in ((EPI_HR, "hr", {}), (EPI_RESID_SSQ, "rs", {}), (EPI_SLOT_STORE, "ss", dict(x_scale=True, mask=True, slot=True))):
            for kz in (1, 2, 4, 8):
                for M in (1, 17, 35):
                    add(spec(f"{tag}_nofullk_kz{kz}_M{M}", "row32", epi, M, 96, 64 * kz, kz=kz, force=1,
                             expect=dict(route=ROUTE_KSPLIT, mode=GM_SLAB, planes=kz, fused=0, split=1), **kw))
        add(spec("join_nofullk", "joiner", EPI_PARTIAL, 17, 96, 256, kz=4, a_op=AOP_TANH_ADD, joiner="ctx", force=1, expect=dict(route=ROUTE_KSPLIT, mode=GM_SLAB, planes=4)))
    for s in out:
        s.knobs = knobs
        assert not s.f16_rows or s.K % (128 * s.kz) == 0, s.name      # (four chunks of whole 32-k blocks per slab)
        if "link" not in s:
            s.link = None
    names = [s.name for s in out]
    assert len(set(names)) == len(names)
    return out


# ------------------------------------------------------------------ the call
IN_FIELDS = ("a0", "a1", "a0b", "aidx0", "aidx1", "aidx0b", "slot_idx", "row_mask", "ctx", "bias", "resid", "p_add", "x_ssq", "r_ssq", "c_state", None, "wp")
OUT_NAMES = ("out", "out16", "state", "state16", "c_state", "ssq", "planes")


def describe(s):
    d = np.zeros(48, np.int32)
    d[:24] = [s.n, s.M, s.N, s.K, s.K0, s.K1, s.kz, s.epi, s.a_op, s.wt, s.waves, s.tile_ok, s.force, s.hidden, s.ldo, s.lda0, s.lda1, s.ldr,
              s.ld_state, s.ldp, -1 if s.run is True else 0, 1, s.vocab, 1]
    d[24:34] = [s.rows_alloc, s.slots, 0, 0, 0, s.xg, s.rg, int(s.out), int(s.out16), int(s.state16)]
    d[34:41] = list(s.tile_pin) + list(s.kw_pin) + list(s.pp_pin)
    return d


def run_case(lib, case):
    """-> (rc, plan dict, [buffers per problem])"""
    s = case.spec
    d = describe(s)
    p0 = case.probs[0]
    d[23] = p0.same_idx_b
    d[26], d[27], d[28] = p0.a0.shape[0], (p0.a1.shape[0] if p0.a1 is not None else 0), (p0.a0b.shape[0] if p0.a0b is not None else 0)
    fd = np.array([1.0 / s.n_norm, s.eps_x, 1.0 / s.n_norm, s.eps_r], np.float32)
    keep, ins, outs, bufs = [], (C.c_void_p * (17 * s.n))(), (C.c_void_p * (7 * s.n))(), []
    for i, p in enumerate(case.probs):
        for j, f in enumerate(IN_FIELDS):
            a = getattr(p, f) if f else None
            if a is not None:
                a = np.ascontiguousarray(a)
                keep.append(a)
                ins[17 * i + j] = a.ctypes.data
        b = {}
        for name, (shape, dtype, *_rest) in R.layout(s, p).items():
            b[name] = np.zeros(shape, dtype)
            outs[7 * i + OUT_NAMES.index(name)] = b[name].ctypes.data
        bufs.append(b)
    plan = np.zeros(16, np.int32)
    rc = lib.aprilx_run_gemm(d.ctypes.data, fd.ctypes.data, ins, outs, plan.ctypes.data)
    return rc, dict(zip(PLAN_KEYS, (int(x) for x in plan))), bufs


def main(knobs, lib=None):
    if lib is None:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        sys.path.insert(0, root)
        from april_asr_amd import _ffi
        lib = _ffi.lib()
    results, done, fault = [], {}, False
    for s in cases(knobs):
        case = R.Case(s)
        if s.link:                                        # a half of a gates GEMM: the inputs of its one-launch form
            kind, whole = s.link
            wcase, wbufs = done[whole]
            for p, wp_ in zip(case.probs, wcase.probs):
                for f in ("W", "wp", "a0", "a1", "aidx1", "slot_idx", "bias", "c_state"):
                    setattr(p, f, getattr(wp_, f))
                p.x_ssq = wp_.x_ssq if kind == "x" else None
                if kind == "h":
                    p.p_add = np.ascontiguousarray(done[whole.replace("_all", "_x")][1][0]["out"][:s.M])      # what the X half left, ldp = ldo
        rc, plan, bufs = run_case(lib, case)
        line = {"name": s.name, "cls": s.cls, "wt": s.wt, "rc": rc, "plan": plan, "ratios": {}, "ok": rc == 0, "why": ""}
        if rc != 0:
            line["why"] = f"aprilx_run_gemm returned {rc}"
        else:
            bad = {k: (plan[k], v) for k, v in s.expect.items() if plan[k] != v}
            if bad:
                line["ok"], line["why"] = False, "plan is not the one the case was written for: " + ", ".join(f"{k} = {a}, expected {b}" for k, (a, b) in bad.items())
            for p, b in zip(case.probs, bufs):
                res = R.compare(s, p, R.evaluate(s, p), b, plan_planes=plan["planes"] if (plan["split"] or s.epi == EPI_PARTIAL) else 0)
                for k, (r, at) in res.items():
                    if r >= line["ratios"].get(k, (-1.0,))[0]:
                        line["ratios"][k] = (r, at)
            w = max((v[0] for v in line["ratios"].values()), default=0.0)
            line["worst"] = w
            if not w <= 1.0:
                line["ok"], line["why"] = False, (line["why"] + "; " if line["why"] else "") + f"err / tol = {w:.3g}"
            if s.link and s.link[0] == "h":               # the halves together give the bits of the one-launch form (kernels.h)
                for k in bufs[0]:
                    if not np.array_equal(R.bits(bufs[0][k]), R.bits(done[s.link[1]][1][0][k])):
                        line["ok"], line["why"] = False, (line["why"] + "; " if line["why"] else "") + f"halves differ from the one-launch form in {k}"
        done[s.name] = (case, bufs)
        if s.link is None and not s.name.endswith("_all"):
            done[s.name] = None
        results.append(line)
        pl = " ".join(f"{k}={plan[k]}" for k in PLAN_KEYS[4:])
        rt = " ".join(f"{k}={v[0]:.3g}@{','.join(map(str, v[1]))}" for k, v in line["ratios"].items())
        print(f"CASE {knobs} {s.name}: {pl} | {rt} | {'ok' if line['ok'] else 'FAIL ' + line['why']}", flush=True)
        if rc == -2:
            fault = True                                  # a HIP call failed (a kernel's fault arrives here, through the synchronize):
            break                                         # nothing more on this GPU, from this process or, by its status, from the parent
    for r in results:
        r["ratios"] = {k: [v[0] if np.isfinite(v[0]) else 1e30, list(v[1])] for k, v in r["ratios"].items()}
        if "worst" in r and not np.isfinite(r["worst"]):
            r["worst"] = 1e30
    print("RESULT " + json.dumps(results), flush=True)
    return HIP_FAILED if fault else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else "default"))
