"""tests/conv_ref.py checked without a GPU: against torch's float64 convolution, against an fp32 emulation of the stated chain, that
the comparison has teeth, and that the host's geometry helpers (csrc/conv_front.h through aprilx_conv_front_geometry) give the sizes
the reference works with.  Also the refusal at load of a front end that needs more shared memory than a launch gets."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as CR      # noqa: E402
import conv_front_worker as W      # noqa: E402

PRODUCT = CR.GEOMETRIES[0]
IDS = ["seg%d_mel%d_s%d%d%d_c%d_%d" % ((g[0], g[1]) + tuple(g[2]) + (g[3], g[4])) for g in CR.GEOMETRIES]


@pytest.mark.parametrize("geo", CR.GEOMETRIES, ids=IDS)
def test_reference_equals_torch_float64(geo):
    import torch
    import torch.nn.functional as F
    s = CR.spec("torch", geo, 2)
    c = CR.Case(s)
    val, _tol = CR.evaluate(s, c)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    dswish = lambda y: y * torch.sigmoid(y - 1.0)
    a1 = dswish(F.conv2d(t(c.x)[:, None], t(c.w0)[:, None], t(c.b0), stride=s.strides[0]))
    a2 = dswish(F.conv2d(a1, t(c.w1), t(c.b1), stride=s.strides[1]))
    assert tuple(a2.shape) == (s.M, s.c1, s.H2, s.W2)
    cols = F.unfold(a2[:, :, :3, :], kernel_size=3, stride=s.strides[2])          # [M][c1 9][W3], k = ci 9 + i 3 + j
    assert tuple(cols.shape) == (s.M, 9 * s.c1, s.W3)
    want = cols.permute(0, 2, 1).reshape(s.M * s.W3, 9 * s.c1).numpy()
    # 1e-12 relative to the array's scale: two float64 summation orders differ by more than that RELATIVE TO AN ELEMENT wherever the
    # terms of a sum cancel (measured: 6e-12 of an element of 1e-4 whose terms are of order one).  Per element, the difference is to
    # be nothing against the tolerance the GPU is judged with.
    assert np.max(np.abs(val - want)) < 1e-12 * np.max(np.abs(want))
    assert np.max(np.abs(val - want) / _tol) < 1e-6


@pytest.mark.parametrize("mode,ring", [("rand", None), ("floor", None), ("sat", None), ("rand", 9)])
@pytest.mark.parametrize("geo", CR.GEOMETRIES, ids=IDS)
def test_fp32_emulation_of_the_stated_chain_lies_inside_the_tolerance(geo, mode, ring):
    if ring:
        ring = geo[0]                                     # a ring of exactly one segment: three of four tails wrap
    s = CR.spec("emu_%s" % mode, geo, 3 if not ring else 4, mode=mode, ring=ring)
    c = CR.Case(s)
    ev = CR.evaluate(s, c)
    res = CR.compare(s, c, ev, CR.render(s, CR.emulate32(s, c)))
    print("emulation %s: err / tol = %.3g" % (s.name, res["ratio"]))
    assert CR.passes(res), res


def teeth_cases():
    ring = CR.spec("teeth_ring", PRODUCT, 4, ring=32 * PRODUCT[0])
    direct = CR.spec("teeth", PRODUCT, 3)
    return {"wrap_off": ring, "no_slot": ring, **{m: direct for m in CR.MUTANTS if m not in ("wrap_off", "no_slot")}}


@pytest.mark.parametrize("mut", CR.MUTANTS)
def test_the_comparison_rejects(mut):
    """kernel row and column swapped; the second conv's patch origin advancing by one, not by the stride, per output index; channel ci
    off by one in conv 2; conv 2's bias dropped; sigma(y) for sigma(y - 1); the rows behind the ring's end read one row further on;
    slot_idx ignored; the im2col k order i 3 + j exchanged for j 3 + i -- each applied to the reference's own output, at the
    product's shape."""
    s = teeth_cases()[mut]
    c = CR.Case(s)
    ev = CR.evaluate(s, c)
    assert CR.passes(CR.compare(s, c, ev, CR.render(s, ev[0])))
    wrong = CR.evaluate(s, c, mut)[0]
    res = CR.compare(s, c, ev, CR.render(s, wrong))
    assert res["ratio"] > 1.0, res
    # not by a hair: most elements are out
    assert (np.abs(wrong - ev[0]) > ev[1]).mean() > (0.5 if mut not in ("wrap_off", "no_slot") else 0.2), mut


def test_exact_parts_have_teeth():
    s = CR.spec("exact", PRODUCT, 3)
    c = CR.Case(s)
    ev = CR.evaluate(s, c)
    good = CR.render(s, ev[0])
    w0t, w1t = CR.transposes(c)
    assert CR.passes(CR.compare(s, c, ev, good, w0t, w1t))
    b = good.copy(); b[s.M * s.W3, 0] = 0.0                                   # a row past M W3
    assert not CR.compare(s, c, ev, b)["fill"]
    b = good.copy(); b[0, 9 * s.c1] = 0.0                                     # a column past 9 c1
    assert not CR.compare(s, c, ev, b)["fill"]
    b = good.copy(); b[0, 2] = np.nextafter(b[0, 2], np.float32(np.inf))      # act2[0][0][0][2] is also element (ow 1, j 0)
    res = CR.compare(s, c, ev, b)
    assert res["ratio"] <= 1.0 and not res["dup"]
    b = good.copy(); b[1, 5] = np.nan
    assert CR.compare(s, c, ev, b)["ratio"] == np.inf
    bad = w1t.copy(); bad[3, 4], bad[4, 3] = bad[4, 3], bad[3, 4]
    assert not CR.compare(s, c, ev, good, w0t, bad)["transposes"]


# ------------------------------------------------------------------ the host's helpers
NP_STATED = {(9, 80, 32): 114, (9, 200, 8): 294, (9, 48, 32): 66, (9, 49, 32): 69, (9, 89, 32): 129}
WIDE = {(9, 80, 32), (9, 48, 32), (9, 49, 32), (10, 64, 32)}                      # the geometries with a many-chunk form


def host_geometry(lib, s):
    d = W.describe(s)
    info = np.zeros(12, np.int32)
    rc = lib.aprilx_conv_front_geometry(d.ctypes.data, info.ctypes.data)
    return rc, info


@pytest.mark.parametrize("geo", CR.GEOMETRIES, ids=IDS)
def test_geometry_table_against_the_host_helpers(built, geo):
    from april_asr_amd import _ffi
    lib = _ffi.lib()
    key = (geo[0], geo[1], geo[4])
    for M in (47, 48):
        s = CR.spec("geom", geo, M, ring=32 * geo[0])
        rc, info = host_geometry(lib, s)
        assert rc == 0
        assert [int(v) for v in info[:8]] == [s.H1, s.W1, s.H2, s.W2, s.W3, s.NP, s.cg, s.lds]
        if key in NP_STATED:
            assert s.NP == NP_STATED[key]
        if "APRIL_CONV_WIDE_MIN" not in os.environ:       # (the knob is read once per process; default: from 48 chunks)
            assert int(info[8]) == int(M >= 48 and key in WIDE), (geo, M)
        assert int(info[9]) == 1
    assert W.path_of(s)["lds"] == s.lds <= 64 * 1024


@pytest.mark.parametrize("geo,why", [((9, 80, (1, 2, 2), 32, 32), 76416), ((9, 255, (1, 2, 2), 8, 32), 77948), ((9, 128, (1, 2, 2), 16, 32), 67008),
                                     ((7, 80, (1, 2, 2), 8, 32), None), ((9, 8, (1, 2, 2), 8, 32), None), ((13, 80, (1, 2, 2), 8, 32), None)])
def test_the_entry_refuses_what_cannot_be_launched(built, geo, why):
    """More than 64 KB of shared memory per workgroup (the sizes stated with the geometry); a segment of 7 rows, which leaves the third
    conv 2 rows; 8 mel bins, which leave it 2 columns; a segment the stack does not reduce to one frame.  aprilx_run_conv_front
    answers -1 the same way before it touches a GPU."""
    from april_asr_amd import _ffi
    lib = _ffi.lib()
    seg, mel, st, c0, c1 = geo
    d = np.zeros(16, np.int32)
    d[:12] = [seg, mel, st[0], st[1], st[2], c0, c1, 1, 9 * c1 + 7, 64, 0, 32 * seg]
    info = np.zeros(12, np.int32)
    assert lib.aprilx_conv_front_geometry(d.ctypes.data, info.ctypes.data) == -1 and int(info[9]) == 0
    if why:
        assert int(info[7]) == why
    import ctypes as C
    ins, outs = (C.c_void_p * 8)(), (C.c_void_p * 3)()
    assert lib.aprilx_run_conv_front(d.ctypes.data, ins, outs, info.ctypes.data) == -1


def test_the_entry_refuses_rows_that_point_outside_the_ring(built):
    from april_asr_amd import _ffi
    lib = _ffi.lib()
    s = CR.spec("bad_rows", PRODUCT, 3, ring=9)
    c = CR.Case(s)
    for field, value in (("slot_idx", s.slots), ("slot_idx", -1), ("tail", s.ring_frames), ("tail", -1)):
        setattr(c, field, getattr(c, field).copy())
        getattr(c, field)[1] = value
        rc, _info, _bufs = W.run_case(lib, c)
        assert rc == -1, (field, value)
        c = CR.Case(s)
    for field, value in (("ldo", 9 * s.c1 - 1), ("out_rows", s.M * s.W3 - 1), ("ring_frames", s.seg - 1), ("M", 0)):
        s2 = CR.Spec(s); s2[field] = value
        info = np.zeros(12, np.int32)
        assert lib.aprilx_conv_front_geometry(W.describe(s2).ctypes.data, info.ctypes.data) == -1, field


# ------------------------------------------------------------------ the refusal at load
@pytest.mark.parametrize("change,words", [(dict(conv_ch=(32, 32, 32)), "76416 bytes of shared memory"), (dict(mel=255), "77948 bytes of shared memory"),
                                          (dict(seg=7), "at least 3 rows")])
def test_a_front_end_that_cannot_run_is_refused_at_load(built, tmp_path, capfd, change, words):
    from april_asr_amd import Model, synth_model as SM
    path = str(tmp_path / "big.april")
    SM.write_model(path, dict(SM.TINY_DIMS, **change), seed=5)
    with pytest.raises(Exception, match="Failed to load model"):
        Model.load_host_only(path)
    err = capfd.readouterr().err
    assert words in err and "conv front end (segment %d, mel %d" % (change.get("seg", 9), change.get("mel", 80)) in err, err


def test_other_geometries_load(built, tmp_path):
    from april_asr_amd import Model, synth_model as SM
    for name, dims, step in W.MODEL_DIMS:
        path = str(tmp_path / (name + ".april"))
        SM.write_model(path, dims, seed=5, params=dict(step=step))
        m = Model.load_host_only(path)
        assert (m.dims.mel, m.dims.seg) == (dims["mel"], dims["seg"])


def test_existing_dims_give_the_same_file_bytes(tmp_path):
    """conv_strides is optional and f_out general: the dims in use write what they wrote before (sha256 of the tiny model's file,
    recorded before the change)."""
    import hashlib
    from april_asr_amd import synth_model as SM
    path = str(tmp_path / "tiny.april")
    SM.write_model(path, SM.TINY_DIMS, seed=5)
    a = open(path, "rb").read()
    SM.write_model(path, dict(SM.TINY_DIMS, conv_strides=(1, 2, 2)), seed=5)
    assert open(path, "rb").read() == a
    assert hashlib.sha256(a).hexdigest() == TINY_SEED5_SHA256


TINY_SEED5_SHA256 = "cc54b33eac3dcb961ab42b928ba75d091ed594c0d4a86a6f120f703147fd68b0"


def test_a_failed_hip_call_ends_the_worker_and_every_later_gpu_process(monkeypatch, capsys):
    """aprilx_run_conv_front returns -2 when a HIP call fails: the worker runs no further case and exits with HIP_FAILED; the parent then
    fails every later test of the module without starting a process.  (No GPU: a library that only answers -2.)"""
    import subprocess
    import test_gpu_conv_front as T

    class Lib:
        calls = 0

        def aprilx_run_conv_front(self, *a):
            Lib.calls += 1
            return -2

    assert W.main("grouped", Lib()) == W.HIP_FAILED and Lib.calls == 1
    out = capsys.readouterr().out
    assert out.count("CASE ") == 1 and "RESULT " in out

    started = []

    def run(cmd, **kw):
        started.append(cmd)
        return subprocess.CompletedProcess(cmd, W.HIP_FAILED, stdout=out.encode(), stderr=b"")

    monkeypatch.setattr(T.subprocess, "run", run)
    monkeypatch.setattr(T, "STATE", {"dead": None, "results": {}})
    with pytest.raises(pytest.fail.Exception, match="status %d" % W.HIP_FAILED):
        T.run_worker("grouped")
    assert len(started) == 1 and T.STATE["dead"]
    with pytest.raises(pytest.fail.Exception, match="not started"):
        T.run_worker("wide")
    with pytest.raises(pytest.fail.Exception, match="not started"):
        T.test_the_cases_that_ran_cover_every_path(None)
    assert len(started) == 1


def test_the_case_lists_reach_every_path_and_every_geometry():
    """What the closing GPU test asserts of the cases that ran holds for the cases as listed."""
    ran = [dict(W.path_of(s), form=f, name=s.name) for knobs in W.KNOB_SETS for s, f in W.cases(knobs)]
    assert not W.missing_paths(ran)
    for knobs in W.KNOB_SETS:
        names = [s.name for s, _f in W.cases(knobs)]
        assert len(set(names)) == len(names)
    grouped = {(s.seg, s.mel, s.strides, s.c0, s.c1) for s, _f in W.cases("grouped")}
    assert grouped >= {(g[0], g[1], tuple(g[2]), g[3], g[4]) for g in CR.GEOMETRIES}
