"""Teardown order of the Python wrapper (no GPU, no library: a stub records the calls).  The C ABI forbids a session to outlive its model.
Sessions whose callbacks refer back to their owner sit in a reference cycle, so they and their model become garbage together; the
collector then clears every weak reference before it runs a finalizer and may finalize the model first.  Model.close() must still free
every open session before the model, and a session finalized after its model must not touch its handle again."""
import gc

import april_asr_amd as A


class StubLib:
    def __init__(self):
        self.calls, self.next = [], 100

    def aas_create_session(self, model, cfg):
        self.next += 1
        return self.next

    def aas_free(self, h):
        self.calls.append(("aas_free", h))

    def aam_free(self, h):
        self.calls.append(("aam_free", h))


class Owner:
    """what a caller typically writes: the callback is a closure over the object that holds the session"""

    def __init__(self, m):
        self.ev = []

        def on_result(t, toks):
            self.ev.append(t)
        self.s = A.Session(m, on_result)


def stub_model(lib):
    m = A.Model.__new__(A.Model)
    m._L, m._handle = lib, 7
    return m


def test_model_and_cyclic_sessions_collected_together():
    lib = StubLib()
    gc.collect()
    gc.disable()
    try:
        m = stub_model(lib)
        owners = [Owner(m) for _ in range(3)]
        handles = [o.s._handle for o in owners]
        del owners, m
        assert lib.calls == []                    # (the cycles keep everything alive until the collector runs)
        gc.collect()
    finally:
        gc.enable()
    assert sorted(c for c in lib.calls if c[0] == "aas_free") == [("aas_free", h) for h in handles]      # each exactly once
    assert lib.calls[-1] == ("aam_free", 7) and lib.calls.count(("aam_free", 7)) == 1                    # ... and all before the model


def test_explicit_close_in_either_order():
    lib = StubLib()
    m = stub_model(lib)
    a, b = A.Session(m, lambda t, toks: None), A.Session(m, lambda t, toks: None)
    ha, hb = a._handle, b._handle
    a.close(); a.close()
    assert lib.calls == [("aas_free", ha)]
    m.close()                                     # closes b, then the model
    assert lib.calls == [("aas_free", ha), ("aas_free", hb), ("aam_free", 7)]
    b.close(); m.close()
    assert len(lib.calls) == 3
