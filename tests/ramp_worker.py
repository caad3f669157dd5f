"""Worker of tests/test_gpu_ramp_merge.py: streams the same sessions and audio through one model four ways in ONE process -- the
pipelined group feed at depth 2 with APRIL_RAMP_MERGE = 0, 1 and 2 (the engine reads the name when a model is created) and the
lock-step group feed once -- and prints, per way, a digest of every callback (token ids, log-probabilities bit for bit, flags,
times; in arrival order per session) with the counters the test asserts on.
usage: ramp_worker.py model.april scenario nsess feeds
scenarios: ms100 | ms120 | ms40 (steady feeds of that length), irregular (30..130 ms, fixed sequence), churn (100 ms feeds; every
fourth feed the eight oldest sessions close and eight new ones open)"""
import ctypes as C
import hashlib
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import april_asr_amd as A  # noqa: E402
from april_asr_amd import synth_model as SM  # noqa: E402

CHURN_EVERY, CHURN_N = 4, 8


def feed_lengths(scenario, feeds):
    if scenario in ("ms100", "churn"):
        return [1600] * feeds
    if scenario == "ms120":
        return [1920] * feeds
    if scenario == "ms40":
        return [640] * feeds
    assert scenario == "irregular", scenario
    out, x = [], 12345
    for _ in range(feeds):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out.append(480 + (x >> 8) % 1601)           # 30 .. 130 ms at 16 kHz: some feeds complete no chunk
    return out


def stream(path, scenario, nsess, feeds, way, pcm_of):
    os.environ["APRIL_RAMP_MERGE"] = {"off": "0", "on": "1", "never": "2", "lockstep": "1"}[way]
    m = A.Model(path)
    events = {}

    def open_session(uid):
        events[uid] = []
        return A.Session(m, lambda t, toks, uid=uid: events[uid].append(
            (int(t), [(x[0], struct.pack("<f", float(x[1])), int(x[2]), int(x[3])) for x in toks])), raw_events=True)

    # who is fed what in every feed, and the pointer / count arrays of every call, before the first one: the feed loop itself is one
    # library call per feed, so the GPU and not this script sets the pace (the next feed's front end then runs beside this feed's layers)
    lengths = feed_lengths(scenario, feeds)
    uids, fed, next_uid, calls = list(range(nsess)), {u: 0 for u in range(nsess)}, nsess, []
    for k, n in enumerate(lengths):
        if scenario == "churn" and k and k % CHURN_EVERY == 0:
            uids = uids[CHURN_N:] + list(range(next_uid, next_uid + CHURN_N))
            for u in range(next_uid, next_uid + CHURN_N):
                fed[u] = 0
            next_uid += CHURN_N
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
        if way == "lockstep":
            grp._L.aprilx_feed_many(nsess, grp._handles, ptrs, cnts)
        else:
            grp._L.aprilx_feed_many_pipelined(nsess, grp._handles, ptrs, cnts, 2)
    grp.drain()
    grp.flush()
    h = hashlib.sha256()
    for uid in sorted(events):
        h.update(repr((uid, events[uid])).encode())
    st = m.stats()
    hosted, eligible = m.ramp_stats()
    print("WAY", way, h.hexdigest(), int(st.chunks), int(st.replay_mismatch), sum(len(e) for e in events.values()), int(st.wave_steps), hosted, eligible, flush=True)
    for s in live.values():
        s.close()
    m.close()


def main():
    path, scenario, nsess, feeds = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
    ways = sys.argv[5].split(",") if len(sys.argv) > 5 else ["off", "on", "never", "lockstep"]
    cache, total = {}, sum(feed_lengths(scenario, feeds))

    def pcm_of(uid):
        if uid not in cache:
            cache[uid] = SM.lcg_pcm16(total, seed=977 + uid)
        return cache[uid]

    for way in ways:
        stream(path, scenario, nsess, feeds, way, pcm_of)


if __name__ == "__main__":
    main()
