"""One process per value of APRIL_CONV_WIDE_MIN (read once per process): runs a list of single launches of the conv front end
(aprilx_run_conv_front) and compares each with tests/conv_ref.py.

    python tests/conv_front_worker.py <knob set>        (the parent sets the knob set's environment)

Prints one line per case -- the form that ran, the worst err / tol, the exact parts -- and a last line RESULT <json> with a digest of
every output (the parent compares the two forms' bytes case by case).  After a failed HIP call (aprilx_run_conv_front returns -2: a
kernel's fault shows up there) it runs no further case and exits with status HIP_FAILED.  The case lists are stated here once;
tests/test_conv_ref_cpu.py walks them without a GPU.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as CR      # noqa: E402

KNOB_SETS = {"grouped": {"APRIL_CONV_WIDE_MIN": "-1"}, "wide": {"APRIL_CONV_WIDE_MIN": "0"}, "default": {}}
HIP_FAILED = 3            # the worker's exit status after a failed HIP call: the parent starts no further GPU process
GROUPED, WIDE = 0, 1
# whole models at other geometries (tests/test_gpu_conv_front.py): name, dims, segment step
_TINY = dict(n_layers=2, d_model=64, hidden=128, ffn=128, joiner=64, vocab=40, context=2, dec_groups=16, conv_ch=(8, 16, 32))
MODEL_DIMS = [("mel40", dict(_TINY, mel=40, seg=9), 4), ("mel128", dict(_TINY, mel=128, seg=9), 4), ("seg11", dict(_TINY, mel=80, seg=11), 4)]


def has_wide(s):
    """The geometries the many-chunk form is instantiated for, as its comment states them: 8 -> 32 channels, H2 = 3, the second
    conv's positions in two waves (64 < NP <= 128)."""
    return s.c0 == 8 and s.c1 == 32 and s.H2 == 3 and 64 < s.NP <= 128


def path_of(s):
    """Which way a geometry takes through the grouped kernel's second conv (how its threads are dealt out over positions and
    channels, read from conv12_kernel) -- used only to say what the cases cover, never to compute a value."""
    per = (s.NP + 63) // 64 * 64
    nsub = 256 // per if per <= 256 else 1
    while nsub > 1 and s.cg % nsub:
        nsub -= 1
    wraps = bool(s.ring and np.any(CR.Case(s).tail + s.seg > s.ring_frames))
    return dict(NP=s.NP, per=per, nsub=nsub, multipass=s.NP > 256, H2=s.H2, cg=s.cg, lds=s.lds, wraps=wraps)


def missing_paths(ran):
    """ran: path_of() + form of every case that ran -> what no case covered."""
    missing = []
    need = lambda what, f: None if any(f(r) for r in ran) else missing.append(what)
    need("the grouped form", lambda r: r["form"] == GROUPED)
    need("the many-chunk form", lambda r: r["form"] == WIDE)
    for n in (1, 2, 3, 4):
        need("nsub %d" % n, lambda r, n=n: r["form"] == GROUPED and r["nsub"] == n)
    need("nsub 1 with 192 positions per subset", lambda r: r["form"] == GROUPED and r["per"] == 192)
    need("the multi-pass loop", lambda r: r["form"] == GROUPED and r["multipass"])
    need("H2 = 4", lambda r: r["H2"] == 4)
    need("a prime channel count", lambda r: r["form"] == GROUPED and r["cg"] == 7)
    for form, name in ((GROUPED, "grouped"), (WIDE, "many-chunk")):
        need("a wrapping tail on the %s form" % name, lambda r, form=form: r["form"] == form and r["wraps"])
    return missing


def cases(knobs):
    """[(spec, the form the case is written for)].  Names are shared between the knob sets: the parent compares the outputs of the
    two forms of one name."""
    out = []
    geos = [CR.spec("g%d" % i, g, 1) for i, g in enumerate(CR.GEOMETRIES)]
    wide_geos = [i for i, g in enumerate(geos) if has_wide(g)]

    def add(name, i, M, **kw):
        s = CR.spec("g%d_%s" % (i, name), CR.GEOMETRIES[i], M, **kw)
        form = WIDE if (has_wide(s) and knobs != "grouped" and (knobs == "wide" or M >= 48)) else GROUPED
        out.append((s, form))

    def ring_cases(i, M):
        seg = CR.GEOMETRIES[i][0]
        for Rf in (32 * seg, seg):
            add("ring%d_M%d" % (Rf, M), i, M, ring=Rf)

    if knobs in ("grouped", "wide"):
        for i in (range(len(geos)) if knobs == "grouped" else wide_geos):
            for M in (1, 3):
                add("M%d" % M, i, M)
        for i in ((0, 2, 5, 6, 9) if knobs == "grouped" else ()) :
            ring_cases(i, 4)
        for i in wide_geos:
            ring_cases(i, 5)
        add("floor_M3", 0, 3, mode="floor")
        add("sat_M3", 0, 3, mode="sat")
        if knobs == "grouped":
            add("floor_M3", 6, 3, mode="floor")
            add("sat_M3", 5, 3, mode="sat")
    if knobs in ("grouped", "default"):
        # the dispatch boundary of the default knob (from 48 chunks); the grouped worker runs the same cases for the digests
        for i in wide_geos:
            for M in (47, 48, 50):
                add("M%d" % M, i, M)
        ring_cases(0, 48)
        add("M48", 13, 48)                                # NP 129: no many-chunk form at any row count
        add("M48", 6, 48)                                 # H2 = 4: neither
    return out


# ------------------------------------------------------------------ the call
def describe(s):
    d = np.zeros(16, np.int32)
    d[:12] = [s.seg, s.mel, s.strides[0], s.strides[1], s.strides[2], s.c0, s.c1, s.M, s.ldo, s.out_rows, s.slots, s.ring_frames]
    return d


def run_case(lib, c):
    """-> (rc, info[12], dict(out, w0t, w1t))"""
    s = c.spec
    d = describe(s)
    ins, outs, keep = (C.c_void_p * 8)(), (C.c_void_p * 3)(), []
    for j, a in enumerate((c.w0, c.b0, c.w1, c.b1, c.x, c.ring, c.slot_idx, c.tail)):
        if a is not None:
            a = np.ascontiguousarray(a, np.int32 if j >= 6 else np.float32)
            keep.append(a)
            ins[j] = a.ctypes.data
    bufs = dict(out=np.zeros((s.out_rows, s.ldo), np.float32), w0t=np.zeros((9, s.c0), np.float32), w1t=np.zeros((9 * s.c0, s.c1), np.float32))
    for j, k in enumerate(("out", "w0t", "w1t")):
        outs[j] = bufs[k].ctypes.data
    info = np.zeros(12, np.int32)
    rc = lib.aprilx_run_conv_front(d.ctypes.data, ins, outs, info.ctypes.data)
    return rc, info, bufs


def main(knobs, lib=None):
    if lib is None:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        sys.path.insert(0, root)
        from april_asr_amd import _ffi
        lib = _ffi.lib()
    results, fault = [], False
    for s, want_form in cases(knobs):
        c = CR.Case(s)
        rc, info, bufs = run_case(lib, c)
        form = int(info[8])
        line = dict(path_of(s), name=s.name, rc=rc, form=form, ok=rc == 0, why="", ratio=None, digest=None)
        if rc != 0:
            line["why"] = "aprilx_run_conv_front returned %d" % rc
        else:
            why = []
            if form != want_form:
                why.append("form %d ran, the case was written for form %d" % (form, want_form))
            res = CR.compare(s, c, CR.evaluate(s, c), bufs["out"], bufs["w0t"], bufs["w1t"])
            line["ratio"], line["at"], line["digest"] = (res["ratio"] if np.isfinite(res["ratio"]) else 1e30), list(res["at"]), CR.digest(bufs["out"])
            if s.mode == "sat":                           # for the record: the same output against the floor at the product alone
                line["product_floor_ratio"] = min(CR.compare(s, c, CR.evaluate(s, c, sigma_floor=False), bufs["out"])["ratio"], 1e30)
            if not res["ratio"] <= 1.0:
                why.append("err / tol = %.3g at %s" % (res["ratio"], res["at"]))
            why += [w for k, w in (("fill", "the fill pattern is broken"), ("dup", "one act2 value has two bit patterns in A3"),
                                   ("transposes", "w0t / w1t are not the transposes")) if not res[k]]
            line["ok"], line["why"] = not why, "; ".join(why)
        results.append(line)
        print("CASE %s %s: form=%d nsub=%d per=%d NP=%d | %s | %s" % (knobs, s.name, form, line["nsub"], line["per"], s.NP,
              ("err/tol=%.3g" % line["ratio"] if line["ratio"] is not None else "-") + (" (floor at the product alone: %.3g)" % line["product_floor_ratio"] if "product_floor_ratio" in line else ""), "ok" if line["ok"] else "FAIL " + line["why"]), flush=True)
        if rc == -2:
            fault = True                                  # a HIP call failed: nothing more on this GPU, from this process or, by its
            break                                         # status, from the parent
    print("RESULT " + json.dumps(results), flush=True)
    return HIP_FAILED if fault else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else "default"))
