"""Worker of tests/test_gpu_ramp_headless.py: tests/ramp_worker.py's sessions, audio and feed loop with the value of APRIL_RAMP_MERGE
given as such (0, 1, 3), so that the deferred enqueue (1) can be set against the guarded head (3) and the parent of both (0), and
with the counters of aprilx_model_ramp_stats2.
usage: ramp_headless_worker.py model.april scenario nsess feeds modes [noclose]
scenarios: those of ramp_worker.py, and switch: 14 feeds of 100 ms (2 / 3 chunks), 12 of 160 ms (4 chunks), 14 of 100 ms again -- three
chunk counts times two flight parities are six launch plans, which a small APRIL_GRAPH_CACHE_CAP cannot hold at once.  modes: comma-separated values of APRIL_RAMP_MERGE, one model each, in ONE process.
noclose: after the last feed call the sessions and the model are closed at once -- no drain, no flush -- so that the last feeds
are still in the air (the very last one possibly with its layer graph deferred) when the library is told to stop.
Prints one line per mode: MODE value digest chunks replay_mismatch callbacks hosted eligible headless settled_wait settled_other"""
import ctypes as C
import hashlib
import os
import struct
import sys

import ramp_worker as RW                                     # (the script's directory is on sys.path)
import april_asr_amd as A
from april_asr_amd import synth_model as SM


def feed_lengths(scenario, feeds):
    if scenario != "switch":
        return RW.feed_lengths(scenario, feeds)
    a = (feeds * 14) // 40
    return [1600] * a + [2560] * (feeds - 2 * a) + [1600] * a


def stream(path, scenario, nsess, feeds, mode, pcm_of, noclose):
    os.environ["APRIL_RAMP_MERGE"] = mode
    m = A.Model(path)
    events = {}

    def open_session(uid):
        events[uid] = []
        return A.Session(m, lambda t, toks, uid=uid: events[uid].append(
            (int(t), [(x[0], struct.pack("<f", float(x[1])), int(x[2]), int(x[3])) for x in toks])), raw_events=True)

    lengths = feed_lengths(scenario, feeds)
    uids, fed, next_uid, calls = list(range(nsess)), {u: 0 for u in range(nsess)}, nsess, []
    for k, n in enumerate(lengths):
        if scenario == "churn" and k and k % RW.CHURN_EVERY == 0:
            uids = uids[RW.CHURN_N:] + list(range(next_uid, next_uid + RW.CHURN_N))
            for u in range(next_uid, next_uid + RW.CHURN_N):
                fed[u] = 0
            next_uid += RW.CHURN_N
        ptrs = (C.c_void_p * nsess)(*[pcm_of(u).ctypes.data + 2 * fed[u] for u in uids])
        cnts = (C.c_size_t * nsess)(*([n] * nsess))
        for u in uids:
            fed[u] += n
        calls.append((list(uids), ptrs, cnts))
    live = {u: open_session(u) for u in calls[0][0]}
    grp = A.SessionGroup([live[u] for u in calls[0][0]])
    for k, (members, ptrs, cnts) in enumerate(calls):
        if k and members != calls[k - 1][0]:
            grp.drain()
            for u in calls[k - 1][0]:
                if u not in members:
                    live.pop(u).close()
            for u in members:
                if u not in live:
                    live[u] = open_session(u)
            grp = A.SessionGroup([live[u] for u in members])
        grp._L.aprilx_feed_many_pipelined(nsess, grp._handles, ptrs, cnts, 2)
    if noclose:
        for s in live.values():
            s.close()
        m.close()
        print("CLOSED", mode, flush=True)
        return
    grp.drain()
    grp.flush()
    h = hashlib.sha256()
    for uid in sorted(events):
        h.update(repr((uid, events[uid])).encode())
    st = m.stats()
    r = m.ramp_stats2()
    print("MODE", mode, h.hexdigest(), int(st.chunks), int(st.replay_mismatch), sum(len(e) for e in events.values()),
          r["hosted"], r["eligible"], r["headless"], r["settled_wait"], r["settled_other"], flush=True)
    for s in live.values():
        s.close()
    m.close()


def main():
    path, scenario, nsess, feeds, modes = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5].split(",")
    noclose = len(sys.argv) > 6 and sys.argv[6] == "noclose"
    cache, total = {}, sum(feed_lengths(scenario, feeds))

    def pcm_of(uid):
        if uid not in cache:
            cache[uid] = SM.lcg_pcm16(total, seed=977 + uid)
        return cache[uid]

    for mode in modes:
        stream(path, scenario, nsess, feeds, mode, pcm_of, noclose)


if __name__ == "__main__":
    main()
