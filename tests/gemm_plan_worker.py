"""Worker for tests/test_gpu_gemm_plan.py: streams the same audio through n sessions of each given model -- eight 100 ms chunk
steps, then one 3 s feed, then a flush -- once with every session's logits traced and once on the untraced (captured-graph) paths,
and prints one digest of all logits and callbacks per model and session count.  The precision comes from the environment."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import april_asr_amd as A  # noqa: E402
from april_asr_amd import synth_model as SM  # noqa: E402

STEPS, LONG = 8, 48000


def run(path, nsess, trace):
    m = A.Model(path)
    events = [[] for _ in range(nsess)]
    sess = []
    for i in range(nsess):
        s = A.Session(m, (lambda t, toks, i=i: events[i].append((int(t), [(x[0], float(x[1]).hex(), int(x[2]), int(x[3])) for x in toks]))), raw_events=True)
        if trace:
            s.trace_logits(3 * 160)
        sess.append(s)
    grp = A.SessionGroup(sess)
    pcm = SM.lcg_pcm16(1600 * STEPS + LONG, seed=4242)
    for k in range(STEPS):
        grp.feed([pcm[1600 * k:1600 * (k + 1)]] * nsess)
    grp.feed([pcm[1600 * STEPS:]] * nsess)
    grp.flush()
    h = hashlib.sha256()
    for i, s in enumerate(sess):
        if trace:
            h.update(np.ascontiguousarray(s.traced_logits()).tobytes())
        h.update(repr(events[i]).encode())
    st = m.stats()
    mismatch, chunks = int(st.replay_mismatch), int(st.chunks)
    for s in sess:
        s.close()
    m.close()
    return h.hexdigest(), chunks, mismatch


def main():
    for path in sys.argv[1:]:
        for nsess in (1, 20, 40):
            for trace in (1, 0):
                d, chunks, mismatch = run(path, nsess, trace)
                print("DIGEST", os.path.basename(path), nsess, trace, d, chunks, mismatch, flush=True)


if __name__ == "__main__":
    main()
