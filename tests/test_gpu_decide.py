"""The device's copy of the search decision (csrc/kernels_misc.hip decide_kernel: the part of aas_process_logits,
reference src/april_session.c:306-429, that the NEXT network call depends on) against the hand-derived fixtures of
tests/golden/state_machine_cases.py and against the host state machine, round by round, with scripted joiner planes injected
through aprilx_run_decide ("a second hand-kept copy ... with no scripted test of its own on the device";
`last_tok >= 0` standing in for `active_token_head > 0` in the digit-dot rule is exercised here)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import state_machine_cases as G  # noqa: E402

import blank_models as BM  # noqa: E402
from april_asr_amd import _ffi  # noqa: E402
from test_state_machine_golden import product_rounds, symbols  # noqa: E402
from test_state_machine import random_triples  # noqa: E402

pytestmark = pytest.mark.gpu
VALID, BLANK, CTX = 1, 2, 4


@pytest.fixture(scope="module")
def gpu_models():
    """engines by model path, loaded once per module"""
    import april_asr_amd as A
    loaded = {}

    def get(path):
        if path not in loaded:
            loaded[path] = A.Model(path)
        return loaded[path]
    yield get
    for m in loaded.values():
        m.close()


class DeviceSearch:
    """One slot's search state on the device, advanced one joiner round at a time through aprilx_run_decide."""

    def __init__(self, model):
        self.L = _ffi.lib()
        self.m = model
        self.V = model.dims.vocab
        self.blank = model.dims.blank_id
        self.state = np.array([self.blank, self.blank, -1, 0], np.int32)

    def round(self, idx, mx, bl, early, now, rnd, tie=None):
        lg = np.full(self.V, -1000.0, np.float32)
        lg[idx] = mx
        if tie is not None:           # an arg-max tie with higher token ids: the device must still report idx (:311-320)
            for t in (tie if isinstance(tie, (tuple, list)) else (tie,)):
                assert t > idx and t != self.blank
                lg[t] = mx
        lg[self.blank] = bl
        nowa = np.array([now], np.int32)
        rec = np.zeros(4, np.uint32)
        before = self.state.copy()
        rc = self.L.aprilx_run_decide(self.m._handle, 1, 0, lg.ctypes.data, C.c_float(early), nowa.ctypes.data, rnd, self.state.ctypes.data, rec.ctypes.data)
        assert rc == 0
        r_idx, r_max, r_bl, flags = int(rec.view(np.int32)[0]), float(rec.view(np.float32)[1]), float(rec.view(np.float32)[2]), int(rec[3])
        assert flags & VALID
        assert r_idx == idx and r_max == np.float32(mx) and r_bl == np.float32(bl)          # the record carries the arg-max and both logits
        changed = (before[0], before[1]) != (self.state[0], self.state[1])
        assert bool(flags & CTX) == changed
        return bool(flags & BLANK)

    def flush(self):
        rc = self.L.aprilx_run_decide(self.m._handle, 1, 1, None, C.c_float(0.0), None, 0, self.state.ctypes.data, None)
        assert rc == 0

    @property
    def ctx(self):
        return (int(self.state[0]), int(self.state[1]))

    @property
    def last_tok(self):
        return int(self.state[2])


def check_hand_derived_case(model, case, sym):
    """one hand-derived case through the device decision (also what tests/device_decide_mutant_worker.py runs against every mutant)"""
    dev = DeviceSearch(model)
    exp = iter(case["rounds"])
    rnd = 0
    for it in product_rounds(case, sym):
        if it[0] == "flush":
            assert next(exp) == "FLUSH"
            dev.flush()
            want_ctx, want_last = case["flush_state"]
            assert dev.ctx == (sym[want_ctx[0]], sym[want_ctx[1]]) and dev.last_tok == (-1 if want_last is None else sym[want_last]), "state after flush"
            continue
        _, idx, mx, bl, early, now, scripted, tie = it
        rnd = 0 if early == 1.0 else rnd + 1
        blank = dev.round(idx, mx, bl, early, now, rnd, tie)
        if not scripted:
            assert blank, "filler round"
            continue
        e = next(exp)
        assert blank == e[0], ("blank flag", case["name"], e)
        assert dev.ctx == (sym[e[1][0]], sym[e[1][1]]), ("context", case["name"], e, dev.ctx)
        assert dev.last_tok == (-1 if e[2] is None else sym[e[2]]), ("last active token", case["name"], e, dev.last_tok)
    assert next(exp, None) is None


@pytest.mark.parametrize("case,which", BM.params(G.CASES, [c["name"] for c in G.CASES], ["blank39"]))
def test_device_decision_matches_hand_derived(gpu_models, request, case, which):
    info = BM.model_info(which, request)
    sym = symbols(info["tokens"])
    model = gpu_models(info["path"])
    assert model.dims.blank_id == info["blank"] == sym["<blk>"]
    check_hand_derived_case(model, case, sym)


@pytest.mark.parametrize("seed,which", BM.params([0, 1], [0, 1], ["blank39", ("blank255", [0])]))
def test_device_decision_matches_host_state_machine_on_random_rounds(gpu_models, request, seed, which):
    """1500 random joiner results per seed (silences, token bursts past 72, punctuation, digits, repeats): the device's
    blank / context decisions equal the host state machine's at every round."""
    info = BM.model_info(which, request)
    model = gpu_models(info["path"])
    L = _ffi.lib()
    rng = np.random.RandomState(100 + seed)
    T = info["tokens"]
    special = [T.index(t) for t in (".", ",", "?", "!", " 1", "2", " 3", "4")]
    triples = random_triples(rng, len(T), 1500, special, blank=info["blank"])
    assert model.dims.blank_id == info["blank"] and all(t[0] != info["blank"] for t in triples)
    h = _ffi.HANDLER(lambda ud, typ, count, toks: None)
    g = L.aprilx_greedy_create(model._handle, h, None)
    dev = DeviceSearch(model)
    ctx = (C.c_int32 * 2)()
    pos, now = 0, 0
    n_blank = n_tok = 0
    while pos < len(triples):
        now += 40
        for r in range(3):
            if pos >= len(triples):
                break
            idx, mx, bl = triples[pos]
            pos += 1
            early = 1.0 if r == 0 else 0.0
            hb = bool(L.aprilx_greedy_step(g, idx, mx, bl, early, now, ctx))
            db = dev.round(idx, mx, bl, early, now, r)
            assert hb == db, (pos, idx, mx, bl, r)
            assert dev.ctx == (int(ctx[0]), int(ctx[1])), (pos, dev.ctx, (ctx[0], ctx[1]))
            n_blank += hb
            n_tok += not hb
            if hb:
                break
    L.aprilx_greedy_free(g)
    assert n_blank > 100 and n_tok > 100


def check_nan_row(model, tokens):
    """A row of NaNs: no logit beats the initial value, the record carries idx == -1 and the decision falls back to a token the
    product chooses (the reference would look up token -1 there): token 1 when the blank is token 0, else token 0.  Decision, context
    and last token equal the host state machine's and bias_ref.Search's, from a cleared context and from live ones."""
    import bias_ref as BR
    L = _ffi.lib()
    V, blank = model.dims.vocab, model.dims.blank_id
    fallback = 1 if blank == 0 else 0
    cls = BR.token_classes([t.encode() for t in tokens])
    sym = symbols(tokens)
    for start in ((blank, blank, -1), (sym["W1"], sym["DOT"], sym["DOT"]), (sym["W1"], fallback, fallback)):
        for bl_is_nan in (True, False):
            row = np.full(V, np.nan, np.float32)
            if not bl_is_nan:
                row[blank] = -5.0
            st = np.array([[start[0], start[1], start[2], 0]], np.int32)
            rec = np.zeros(1, np.dtype([("idx", np.int32), ("max", np.float32), ("blank", np.float32), ("flags", np.uint32)]))
            nowa = np.array([40], np.int32)
            assert L.aprilx_run_decide(model._handle, 1, 0, row.ctypes.data, C.c_float(1.0), nowa.ctypes.data, 0, st.ctypes.data, rec.ctypes.data) == 0
            assert int(rec["idx"][0]) == -1 and rec["flags"][0] & VALID, "NaN row: idx"
            assert np.isnan(rec["blank"][0]) == bl_is_nan, "NaN row: blank logit"
            # bias_ref.Search: the decision kernel's statement
            srch = BR.Search(cls, blank, None)
            srch.ctx, srch.last_tok = [start[0], start[1]], start[2]
            idx, mx, bl, want_blank = srch.step(row, 1.0, 40)
            assert idx == -1
            # the host state machine, brought to the same state by emitting the context's tokens first
            h = _ffi.HANDLER(lambda ud, typ, count, toks: None)
            g = L.aprilx_greedy_create(model._handle, h, None)
            ctx = (C.c_int32 * 2)()
            if start[2] >= 0:
                for t in start[:2]:
                    assert not L.aprilx_greedy_step(g, t, 50.0, -50.0, 0.0, 0, ctx)
                assert (ctx[0], ctx[1]) == start[:2]
            hb = bool(L.aprilx_greedy_step(g, -1, float(mx), float(bl), 1.0, 40, ctx))
            L.aprilx_greedy_free(g)
            assert bool(rec["flags"][0] & BLANK) == want_blank == hb, ("NaN row: decision", start, bl_is_nan, int(rec["flags"][0]), want_blank, hb)
            assert (int(st[0][0]), int(st[0][1])) == tuple(srch.ctx) == (int(ctx[0]), int(ctx[1])), ("NaN row: context", start, bl_is_nan, list(st[0]), srch.ctx, (ctx[0], ctx[1]))
            assert int(st[0][2]) == srch.last_tok, ("NaN row: last token", start, bl_is_nan)
            if not want_blank:
                assert int(st[0][1]) == fallback and int(st[0][2]) == fallback, "NaN row: the fallback token"


@pytest.mark.parametrize("which", ["tiny", "blank39"])
def test_nan_row(gpu_models, request, which):
    """blank39: the `0` arm of `a.blank == 0 ? 1 : 0`, which no blank-0 model reaches"""
    info = BM.model_info(which, request)
    model = gpu_models(info["path"])
    assert model.dims.blank_id == info["blank"]
    check_nan_row(model, info["tokens"])


def check_same_lane_ties(model):
    """Lane t of the arg-max loop owns n = t, t + 256, ...: a tie between two of ITS ids goes to the lower one only because ids ascend
    within a lane and the comparison is `>` (V = 500: two ids per lane at most).  As the maximum, below the blank, above it."""
    V, blank = model.dims.vocab, model.dims.blank_id
    assert V >= 500
    dev = DeviceSearch(model)
    lows = [n for n in (1, 17, 63, 64, 200, 243) if n != blank and n + 256 != blank and n + 256 < V]
    assert len(lows) >= 5
    now = 0
    for n in lows:
        for bl in (-10.0, 10.0):
            now += 40
            is_blank = dev.round(n, 5.0, bl, 1.0, now, 0, tie=n + 256)        # (round() asserts that the record names n)
            assert is_blank == (bl > 5.0), "same-lane tie: decision"
            if not is_blank:
                assert dev.ctx[1] == n and dev.last_tok == n, "same-lane tie: context"
    # ... and tie partners in another lane of the same wave / in another wave, beside the one of its own lane
    now += 40
    dev.round(17, 5.0, -10.0, 1.0, now, 0, tie=(18, 81, 273, 274))
    assert dev.ctx[1] == 17


@pytest.mark.parametrize("which", ["v0", "blank255"])
def test_ties_between_ids_of_one_lane(gpu_models, request, which):
    info = BM.model_info(which, request)
    model = gpu_models(info["path"])
    assert model.dims.vocab == 500 and model.dims.blank_id == info["blank"]
    check_same_lane_ties(model)


def test_every_mutant_of_the_device_decision_is_killed(built, tiny_model, request):
    """30 single-edit mutants of decide_kernel (csrc/kernels_misc.hip: tie order between lanes and inside one, the comparisons and constants of the
    blank decision, the punctuation override and the digit-dot rule, the context push, the silence rule, the blank id's uses), each compiled and
    linked into its own library on this box and run through aprilx_run_decide against the hand-derived cases on the tiny model and on blank39, the
    NaN row and the same-lane ties on blank255 (tests/mutate_device_decide.py): none may pass them all -- the device's copy is the third
    transcription of src/april_session.c:306-429 beside the oracle's and the host's"""
    import mutate_device_decide as DM
    killed, survivors, eq_killed, failures = DM.run_all(model_path=tiny_model["path"], blank39_path=BM.model_info("blank39", request)["path"],
                                                        ties_path=BM.model_info("blank255", request)["path"])
    assert not failures, failures
    assert not survivors, "mutants of decide_kernel that pass every hand-derived case: %r" % [n for n, _ in survivors]
    assert not eq_killed, "mutants listed as equivalent that a case does catch (the argument is wrong): %r" % eq_killed
    assert len(killed) == len(DM.MUTANTS) >= 30


def test_every_mutant_of_the_opt_in_lines_is_killed(built, request):
    """Single-edit mutants of the lines only the opt-in forms run -- bias_scan, bias_apply, bias_row_begin, bias_row_end and the strict sets
    (csrc/kernels_bias.inc), the OPT lines of decide_body, confidence_row (csrc/kernels_confidence.inc) --, each built into its own library and
    run against bias_ref, bias_strict_ref, search_options_ref and confidence_ref on blank39 and blank1050 by the code of the kernel-level tests
    (tests/device_optin_mutant_worker.py): none may pass, and every mutant listed as equivalent must."""
    import mutate_device_decide as DM
    killed, survivors, eq_killed, failures = DM.run_optin(blank39_path=BM.model_info("blank39", request)["path"],
                                                          blank1050_path=BM.model_info("blank1050", request)["path"])
    assert not failures, failures
    assert not survivors, "mutants of the opt-in lines that pass every reference-based check: %r" % [n for n, _ in survivors]
    assert not eq_killed, "mutants listed as equivalent that a check does catch (the argument is wrong): %r" % eq_killed
    assert len(killed) == len(DM.OPTIN_MUTANTS) >= 36 and len(DM.OPTIN_EQUIVALENT) >= 4
