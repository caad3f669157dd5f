"""Helpers of tests/test_search_options_cpu.py and tests/test_gpu_search_options.py, and -- run as a program -- the worker of
tests/mutate_search_options.py: every hand-derived case of tests/golden/search_options_cases.py through the host state machine
(csrc/session.cc `Greedy`, aprilx_greedy_*) of the library named by APRIL_ASR_LIB.  Host-only (no GPU).
    python search_options_worker.py MODEL.april      prints SURVIVED and exits 0 when every case passes, else "KILLED by <case>" and exits 1."""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE), os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import search_options_cases as G  # noqa: E402

KIND = {"PARTIAL": 1, "FINAL": 2, "SILENCE": 4}


def symbols(tokens):
    """the fixtures' vocabulary symbols -> token ids (the rule of tests/test_state_machine_golden.py)"""
    tokens = [t.decode() if isinstance(t, bytes) else t for t in tokens]

    def first(pred, skip=()):
        return next(i for i, t in enumerate(tokens) if i not in skip and pred(t))
    w1 = first(lambda t: t.startswith(" ") and len(t) > 2 and not t[1].isdigit())
    w2 = first(lambda t: t.startswith(" ") and len(t) > 2 and not t[1].isdigit(), (w1,))
    c1 = first(lambda t: not t.startswith(" ") and t.isalpha() and len(t) > 1)
    c2 = first(lambda t: not t.startswith(" ") and t.isalpha() and len(t) > 1, (c1,))
    return {"W1": w1, "W2": w2, "C1": c1, "C2": c2, "DOT": tokens.index("."), "COMMA": tokens.index(","), "D2": tokens.index("2"), "<blk>": tokens.index("<blk>")}


def make_options(opts, size_delta=0):
    from april_asr_amd import _ffi
    E, p, U = opts
    return _ffi.AprilxSearchOptions(C.sizeof(_ffi.AprilxSearchOptions) + size_delta, int(E), int(U), float(p))


def want_events(case, sym):
    return [(KIND[k], [(sym[s], float(lp), int(fl), int(t)) for (s, lp, fl, t) in toks]) for k, toks in case["events"]]


class ProductGreedy:
    """aprilx_greedy_* with the events collected as (type, [(token id, logprob, flags, time_ms)])"""

    def __init__(self, model, opts=None):
        from april_asr_amd import _ffi
        self.L = _ffi.lib()
        self.events = []
        tok_index = {model.token(i).encode(): i for i in range(model.dims.vocab)}

        def handler(ud, typ, count, toks):
            self.events.append((int(typ), [(tok_index[toks[i].token], float(toks[i].logprob), int(toks[i].flags), int(toks[i].time_ms)) for i in range(count)]))
        self._h = _ffi.HANDLER(handler)
        self.g = self.L.aprilx_greedy_create(model._handle, self._h, None)
        self.ctx = (C.c_int32 * 2)()
        if opts is not None:
            assert self.set(opts) == 0

    def set(self, opts, size_delta=0):
        if opts is None:
            return self.L.aprilx_greedy_set_search_options(self.g, None)
        return self.L.aprilx_greedy_set_search_options(self.g, C.byref(make_options(opts, size_delta)))

    def step(self, idx, mx, bl, early, now):
        blank = bool(self.L.aprilx_greedy_step(self.g, int(idx), float(mx), float(bl), float(early), int(now), self.ctx))
        return blank, (int(self.ctx[0]), int(self.ctx[1]))

    def finish(self):
        self.L.aprilx_greedy_finish(self.g)

    def close(self):
        self.L.aprilx_greedy_free(self.g)


def check_product_case(case, model, sym):
    g = ProductGreedy(model, case["opts"])
    try:
        for i, ((s, mx, bl, early, now), exp) in enumerate(zip(case["rounds"], case["expect"])):
            got = g.step(sym[s], mx, bl, early, now)
            assert got == (exp[0], (sym[exp[1][0]], sym[exp[1][1]])), (case["name"], "round", i, got, exp)
        want = want_events(case, sym)
        assert [e[0] for e in g.events] == [e[0] for e in want], (case["name"], "event types", [e[0] for e in g.events], [e[0] for e in want])
        for i, (a, b) in enumerate(zip(g.events, want)):
            assert a == b, (case["name"], "event", i, a, b)
    finally:
        g.close()


def main():
    import april_asr_amd as A
    m = A.Model.load_host_only(sys.argv[1])
    sym = symbols([m.token(i) for i in range(m.dims.vocab)])
    for case in G.CASES:
        try:
            check_product_case(case, m, sym)
        except AssertionError as e:
            print("KILLED by %s: %s" % (case["name"], str(e)[:200]))
            return 1
    print("SURVIVED")
    return 0


if __name__ == "__main__":
    sys.exit(main())
