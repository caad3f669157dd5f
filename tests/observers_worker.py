"""Worker for tests/test_gpu_observers.py: sixteen sessions of one group, one per subset of {voice activity, DTMF, tones, line quality},
all fed the same samples through the same group feeds.  Prints one line "RESULT <json>".
usage: observers_worker.py model.april"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  -- first, so the process uses ONE HIP runtime
import april_asr_amd as A  # noqa: E402
import vad_ref as V  # noqa: E402
import dtmf_ref as D  # noqa: E402
import tone_ref as T  # noqa: E402
from quality_worker import Run, geometry  # noqa: E402

OBSERVERS = ("vad", "dtmf", "tones", "quality")    # bit x of a session's mask: observer x is on (the block's order)
SECONDS = 1.5
BURST = (0.15, 0.55)                               # quality_worker's all4 scenario: a burst that trips voice activity ...
KEY = ("7", 0.30)                                  # ... with a key inside it
TONE = (1100, 0.65, 0.25)                          # one call-progress tone behind it
CLIPPED = (1.00, 1.10)                             # a 440 Hz sine driven into the rails
DEAD = (1.20, 1.45)                                # digital silence
QUALITY = dict(clip_level=20000, clip_run_min=2, clip_hold_ms=100, dropout_ms=20, report_ms=250)


def audio(sr):
    sig = V.burst_signal(SECONDS, [BURST], -50.0, 20.0, seed=50).astype(np.int32)
    key, onsets = D.digit_signal(KEY[0], 100, 0, sr, -200.0, seed=0, tail_ms=0)
    a = int(KEY[1] * sr)
    sig[a:a + sr // 10] += key[onsets[0]:onsets[0] + sr // 10]
    a, n = int(TONE[1] * sr), int(TONE[2] * sr)
    sig[a:a + n] += T.to_pcm(T.sine(TONE[0], n, sr, -12.0)).astype(np.int32)
    a, b = int(CLIPPED[0] * sr), int(CLIPPED[1] * sr)
    sig[a:b] += np.round(4.0 * 32768.0 * np.sin(2 * np.pi * 440.0 * np.arange(b - a) / float(sr))).astype(np.int32)
    pcm = np.clip(sig, -32768, 32767).astype(np.int16)
    pcm[int(DEAD[0] * sr):int(DEAD[1] * sr)] = 0
    return pcm


def main():
    m = A.Model(sys.argv[1])
    sr = geometry(m)[0]
    assert sr == 16000
    pcm = audio(sr)
    on = [[bool(mask >> x & 1) for x in range(4)] for mask in range(16)]
    runs = [Run(m, vad=o[0] or None, dtmf=o[1] or None, tones=o[2] or None, quality=QUALITY if o[3] else None) for o in on]
    grp = A.SessionGroup([r.s for r in runs])
    for a in range(0, len(pcm), sr // 10):
        grp.feed([pcm[a:a + sr // 10]] * len(runs))
    grp.flush(); grp.drain()
    events = dict(vad=[[list(e) for e in r.vad] for r in runs], dtmf=[[list(e) for e in r.keys] for r in runs],
                  tones=[[list(e) for e in r.tones] for r in runs], quality=[[list(e) for e in r.q] for r in runs])
    info = dict(vad=[r.s.vad_info() for r in runs], dtmf=[r.s.dtmf_info() for r in runs], tones=[r.s.tone_info() for r in runs],
                quality=[r.s.quality() for r in runs])
    out = dict(events=events, info=info, tokens_equal=[r.ev == runs[0].ev for r in runs], n_token_events=len(runs[0].ev),
               chunks=[r.s.chunks() for r in runs], mismatch=int(m.stats().replay_mismatch))
    for r in runs:
        r.s.close()
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
