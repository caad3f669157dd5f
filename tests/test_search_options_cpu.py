"""Per-session search options without a GPU: the host state machine (csrc/session.cc `Greedy`, through
aprilx_greedy_*) against the hand-derived cases of tests/golden/search_options_cases.py and against the reference statement
tests/search_options_ref.py; defaults against the 21 existing state-machine fixtures; refusals; single-edit mutants of the new host lines."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import search_options_cases as G  # noqa: E402
import state_machine_cases as SMC  # noqa: E402

import april_asr_amd as A  # noqa: E402
import blank_models as BM  # noqa: E402
import search_options_ref as R  # noqa: E402
import search_options_worker as W  # noqa: E402


@pytest.fixture(scope="module")
def host_model(tiny_model):
    m = A.Model.load_host_only(tiny_model["path"])
    yield m
    m.close()


@pytest.fixture(scope="module")
def sym(tiny_model):
    return W.symbols(tiny_model["tokens"])


def test_the_cases_cover_what_the_contract_names():
    names = [c["name"] for c in G.CASES]
    assert len(set(names)) == len(names)
    for E in (200, 700, 2200, 60000):
        assert "endpoint_boundary_%d" % E in names
    for c in G.CASES:
        assert len(c["rounds"]) == len(c["expect"])
        assert c["opts"] is None or R.accepted(*c["opts"])
    assert np.float32(G.UP_6_5) == np.nextafter(np.float32(6.5), np.float32(np.inf))
    assert np.float32(np.float32(G.UP_6_5) - np.float32(1.5)) == np.nextafter(np.float32(5.0), np.float32(np.inf))


CASE_PARAMS = BM.params(G.CASES, [c["name"] for c in G.CASES], ["blank39"])


@pytest.fixture(scope="module")
def blank39(request):
    info = BM.model_info("blank39", request)
    m = A.Model.load_host_only(info["path"])
    assert m.dims.blank_id == 39
    yield dict(info, model=m, sym=W.symbols(info["tokens"]))
    m.close()


@pytest.mark.parametrize("case,which", CASE_PARAMS)
def test_product_matches_hand_derived(built, host_model, sym, blank39, case, which):
    if which == "blank39":
        host_model, sym = blank39["model"], blank39["sym"]
        assert sym["<blk>"] == 39
    W.check_product_case(case, host_model, sym)


@pytest.mark.parametrize("case,which", CASE_PARAMS)
def test_reference_statement_matches_hand_derived(tiny_model, sym, blank39, case, which):
    """tests/search_options_ref.py (what the GPU tests replay live sessions with) on the same cases: events, decisions, device state"""
    info = blank39 if which == "blank39" else dict(tiny_model, blank=0)
    sym = blank39["sym"] if which == "blank39" else sym
    blank = info["blank"]
    cls = R.token_classes(info["tokens"])
    g, s = R.Greedy(cls, blank, case["opts"]), R.Search(cls, blank, case["opts"])
    for i, ((t, mx, bl, early, now), exp) in enumerate(zip(case["rounds"], case["expect"])):
        is_blank = g.step(sym[t], mx, bl, early, now)
        d_blank, _, changed = s.step(sym[t], mx, bl, early, now)
        assert is_blank == d_blank == exp[0], (case["name"], i)
        assert g.ctx == s.ctx == [sym[exp[1][0]], sym[exp[1][1]]], (case["name"], i)
        assert s.last_tok == (-1 if exp[2] is None else sym[exp[2]]) and s.last_emit == exp[3] and changed == exp[4], (case["name"], i)
    assert g.events == W.want_events(case, sym), case["name"]


def test_penalty_of_zero_keeps_the_bits():
    """bl - 0.0f is bl for every non-NaN bl (section 14): the sign of zero, denormals, infinities included"""
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32).view(np.float32),
                        np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45], np.float32)])
    v = v[~np.isnan(v)]
    assert np.array_equal((v - np.float32(0.0)).view(np.uint32), v.view(np.uint32))


def test_defaults_equal_no_options_on_the_existing_fixtures(built, tiny_model, host_model):
    """E = 2200, p = 0, U = 0 set explicitly: the events and decisions of the 21 state-machine fixtures are those of a Greedy without options"""
    from test_state_machine_golden import product_rounds, symbols
    assert len(SMC.CASES) == 21
    sym = symbols(tiny_model["tokens"])
    for case in SMC.CASES:
        runs = []
        for opts in (None, (2200, 0.0, 0)):
            g = W.ProductGreedy(host_model, opts)
            decisions = []
            for it in product_rounds(case, sym):
                if it[0] == "flush":
                    g.finish()
                    continue
                decisions.append(g.step(it[1], it[2], it[3], it[4], it[5]))
            runs.append((g.events, decisions))
            g.close()
        assert runs[0][0], case["name"]
        assert runs[0] == runs[1], case["name"]


def test_refused_values_change_nothing(built, host_model, sym):
    """The refusals by value and by `size`, through aprilx_greedy_set_search_options, which has no getter: that the previous options stay in
    place is shown by behaviour (the E = 700 boundary case still passes afterwards).  The session-level half of the issue's list -- the same
    refusals through aprilx_session_set_search_options with the previous options read back through aprilx_session_search_options, and the
    refusal for a session with audio fed since its last flush -- needs a session, and a session needs an engine: it is in
    tests/test_gpu_search_options.py::test_life_cycle."""
    case = next(c for c in G.CASES if c["name"] == "endpoint_boundary_700")
    g = W.ProductGreedy(host_model, (700, 0.0, 0))
    for E, p, U, dsize in G.REFUSED:
        assert not (R.accepted(E, p, U) and dsize == 0)
        assert g.set((E, p, U), dsize) == -1, (E, p, U, dsize)
    for (t, mx, bl, early, now), exp in zip(case["rounds"], case["expect"]):       # still E = 700
        assert g.step(sym[t], mx, bl, early, now)[0] == exp[0]
    assert g.events == W.want_events(case, sym)
    for o in G.ACCEPTED:
        assert R.accepted(*o) and g.set(o) == 0, o
    assert g.set(None) == 0
    g.close()


def test_every_mutant_of_the_new_host_lines_is_killed(built, tiny_model):
    import mutate_search_options as M
    killed, survivors, failures = M.run_all(model_path=tiny_model["path"])
    assert not failures, failures
    assert not survivors, "mutants that no search-option case catches: %s" % [n for n, _ in survivors]
    assert len(killed) == len(M.MUTANTS) == 9
