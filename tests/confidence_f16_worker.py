"""Child process of tests/test_gpu_confidence.py::test_f16_engine, started with APRIL_PRECISION=f16: the confidences of a session
on the fp16 engine alone == the same session in a batch of 24 (bit for bit), and inside the bound of DESIGN.md section 12 against the
fp16 engine's OWN traced logits.  Needs a GPU.  Prints F16_CONFIDENCE_OK and exits 0 when everything holds."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    import torch  # noqa: F401  -- first, as in conftest.py: one HIP runtime for torch and the library
    import april_asr_amd as A
    from oracle import orc_py as O
    from test_gpu_confidence import check_live, live_pcm, run
    gm = A.Model(sys.argv[1])
    assert gm.dims.precision == 1, "the engine is not in fp16-operand mode"
    pcm = live_pcm("v0")
    ev_t, log_t, lg = run(gm, pcm, 1600, 4, trace=True)
    n_tok, n_final2, n_prov, worst = check_live(ev_t, log_t, lg, gm.dims.blank_id, 4)
    assert n_tok > 0
    ev1, log1, _ = run(gm, pcm, 1600, 4)
    assert (ev1, log1) == (ev_t, log_t), "fp16 engine: eager and graph-replayed steps differ"
    n = 24
    pcms = [pcm] + [O.lcg_pcm16_fast(pcm.size, seed=700 + i) for i in range(1, n)]
    evs = [[] for _ in range(n)]
    ss = [A.Session(gm, (lambda q: (lambda t, toks: evs[q].append((t, toks))))(i), raw_events=True, alternatives=(4 if i % 3 == 0 else None)) for i in range(n)]
    ss[0].info_log = []
    g = A.SessionGroup(ss)
    for o in range(0, pcm.size, 1600):
        g.feed([p[o:o + 1600] for p in pcms])
    g.flush()
    assert gm.stats().replay_mismatch == 0
    assert evs[0] == ev1 and ss[0].info_log == log1, "fp16 engine: a session's confidences depend on its neighbours"
    for s in ss:
        s.close()
    gm.close()
    print("fp16 engine: %d tokens inside the bound against its own logits (worst %.3f of it), alone == in a batch of %d" % (n_tok, worst, n))
    print("F16_CONFIDENCE_OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
