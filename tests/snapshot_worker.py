"""Worker for tests/test_gpu_snapshot.py: session snapshot and restore (aprilx_session_snapshot / aprilx_session_restore and the
batched forms), one scenario per process.  Prints one line "RESULT <json>".
usage: snapshot_worker.py model.april mode [args ...]

Every comparison is exact and is made against the UNINTERRUPTED run of the same audio in the same feed sizes: the source that went on
after its snapshot and the restored copy must deliver what that run delivered after the cut -- token callbacks (logprob by bits),
AprilxTokenInfo bytes, VAD / DTMF / tone events, feature rows, contexts, trie states, counters."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  -- first, so the process uses ONE HIP runtime
import april_asr_amd as A  # noqa: E402
from april_asr_amd import _ffi  # noqa: E402
import snapshot_ref as R  # noqa: E402
import dtmf_ref as D  # noqa: E402
import tone_ref as TR  # noqa: E402
import input_format_ref as IF  # noqa: E402
from conftest import speech_like_pcm  # noqa: E402
from bias_worker import model_texts, session_phrases  # noqa: E402

PARTIAL, FINAL = 1, 2


def bits(x):
    return int(np.float32(x).view(np.uint32))


class Stream:
    """a session that writes down everything it delivers, in order, as JSON-able values"""

    def __init__(self, gm, asynchronous=False, **cfg):
        self.log = []
        self.s = A.Session(gm, self._tok, raw_events=True, asynchronous=asynchronous,
                           vad_callback=lambda e: self.log.append(["vad", e.kind, e.time_ms]),
                           dtmf_callback=lambda e: self.log.append(["dtmf", e.kind, e.digit, e.time_ms]),
                           tone_callback=lambda e: self.log.append(["tone", e.kind, e.f1_hz, e.f2_hz, e.time_ms]), **cfg)
        self.s.info_log = [] if cfg.get("alternatives") else None
        self.hook = None

    def _tok(self, t, toks):
        infos = None
        if self.s.info_log is not None:
            infos = [hashlib.sha1(b).hexdigest() if b is not None else None for b in self.s.info_log.pop()[1]]
        self.log.append(["tok", int(t), [[k[0].decode("latin1"), bits(k[1]), k[2], k[3]] for k in toks], infos])
        if self.hook:
            self.hook()

    def feed(self, data, bounds):
        for a, b in bounds:
            self.s.feed(data[a:b])

    def rows_written(self):
        return int(self.s._L.aprilx_session_read_frames(self.s._handle, 0, 0, None))

    def rows(self, first, n=None):
        """feature rows [first, first + n) (to the end without n) as float32 [n][mel]"""
        total = self.rows_written()
        n = total - first if n is None else n
        out = np.zeros((n, self.s.model.dims.mel), np.float32)
        if n:
            got = int(self.s._L.aprilx_session_read_frames(self.s._handle, first, n, out.ctypes.data))
            assert got == total, (got, total, first, n)
        return out

    def state(self):
        h, d = self.s.contexts()
        return dict(chunks=self.s.chunks(), frames_seen=self.s.frames_seen(), rows_written=self.rows_written(), ctx=h.tolist(), dev=d.tolist(), bias=list(self.s.bias_state()),
                    vad=self.s.vad_info(), dtmf=self.s.dtmf_info(), tones=self.s.tone_info())


def bounds(lo, hi, feed):
    return [(a, min(a + feed, hi)) for a in range(lo, hi, feed)]


def digest(rows):
    return hashlib.sha1(np.ascontiguousarray(rows).tobytes()).hexdigest()


def count(log, kind):
    return sum(1 for e in log if e[0] == "tok" and e[1] == kind)


def uninterrupted(gm, cfg, data, feed, cut, flush_at_cut=False):
    """the reference side: the whole audio with a feed boundary at the cut.  Returns what the comparisons need, and closes the session."""
    u = Stream(gm, **cfg)
    u.feed(data, bounds(0, cut, feed))
    if flush_at_cut:
        u.s.flush()
    mark, at_cut = len(u.log), u.state()
    u.feed(data, bounds(cut, len(data), feed))
    u.s.flush()
    before = [e for e in u.log[:mark] if e[0] == "tok"]
    ref = dict(mark=mark, log=u.log, at_cut=at_cut, end=u.state(), rows=digest(u.rows(at_cut["rows_written"])), n_rows=u.rows_written() - at_cut["rows_written"],
               finals_after=count(u.log[mark:], FINAL), partials_after=count(u.log[mark:], PARTIAL),
               active_at_cut=len(before[-1][2]) if before and before[-1][1] == PARTIAL else 0, bias_at_cut=at_cut["bias"][0],
               kinds_before=sorted({e[0] for e in u.log[:mark]}), kinds_after=sorted({e[0] for e in u.log[mark:]}))
    u.s.close()
    return ref


def compare(name, ref, stream, log_from, bad):
    """`stream` after the end of the audio against the uninterrupted run: what it delivered since the cut, its feature rows since the cut, its state"""
    if stream.log[log_from:] != ref["log"][ref["mark"]:]:
        bad.append("%s: callbacks after the cut differ (%d against %d)" % (name, len(stream.log) - log_from, len(ref["log"]) - ref["mark"]))
    if stream.state() != ref["end"]:
        bad.append("%s: state at the end differs: %r against %r" % (name, stream.state(), ref["end"]))
    if digest(stream.rows(ref["at_cut"]["rows_written"])) != ref["rows"]:
        bad.append("%s: feature rows after the cut differ" % name)


def three(gm, cfg, data, feed, cut, flush_at_cut=False, target_cfg=None):
    """uninterrupted run, source that goes on after its snapshot, restored copy: returns (what the reference side showed, mismatches, blob)"""
    ref = uninterrupted(gm, cfg, data, feed, cut, flush_at_cut)
    bad = []
    s = Stream(gm, **cfg)
    s.feed(data, bounds(0, cut, feed))
    if flush_at_cut:
        s.s.flush()
    if s.log != ref["log"][:ref["mark"]] or s.state() != ref["at_cut"]:
        bad.append("source differs from the uninterrupted run BEFORE the cut")
    blob = s.s.snapshot()
    if s.state() != ref["at_cut"]:
        bad.append("the snapshot changed the source")
    t = Stream(gm, **(target_cfg or cfg))
    t.s.restore(blob)
    if t.state() != ref["at_cut"]:
        bad.append("restored state differs at the cut: %r against %r" % (t.state(), ref["at_cut"]))
    p = R.parse(blob)
    avail = p["book"]["avail"]
    if avail and digest(t.rows(ref["at_cut"]["rows_written"] - avail, avail)) != digest(s.rows(ref["at_cut"]["rows_written"] - avail, avail)):
        bad.append("the ring rows the book still names differ on the copy")
    rest = bounds(cut, len(data), feed)
    s.feed(data, rest); s.s.flush()
    t.feed(data, rest); t.s.flush()
    compare("source", ref, s, ref["mark"], bad)
    compare("copy", ref, t, 0, bad)
    # the control: a fresh session fed the same remaining audio WITHOUT the blob -- where it delivers something else, the comparison above tells states apart
    c = Stream(gm, **(target_cfg or cfg))
    c.feed(data, rest); c.s.flush()
    texts = lambda log: [[e[1], [k[0] for k in e[2]]] for e in log if e[0] == "tok"]      # noqa: E731  (its clocks start at 0: only types and token texts)
    ref["control_differs"] = texts(c.log) != texts(ref["log"][ref["mark"]:])
    c.s.close()
    ref.update(avail=avail, tail_bytes=len(p["book"]["audio"]), blob_bytes=len(blob), head=p["search"]["head"], seg=p["book"]["seg_count"],
               src_ring=p["book"]["ring_frames"], rows_at_cut=ref["at_cut"]["rows_written"], mismatch=gm.stats().replay_mismatch)
    s.s.close(); t.s.close()
    out = {k: v for k, v in ref.items() if k not in ("log", "at_cut", "end")}
    return out, bad, blob


def all_cfg(gm, seed=3):
    texts = model_texts(gm)
    bias = gm.bias(session_phrases(texts, gm.dims.blank_id, np.random.default_rng(seed)))
    cfg = dict(input_sample_rate=8000, input_format="mulaw", alternatives=4, bias=bias, endpoint_silence_ms=600, blank_penalty=0.5, max_utterance_ms=2000,
               vad=dict(onset_ms=40), dtmf=True, tones=dict(min_tone_ms=80))
    return cfg, bias


def all_audio():
    """8 kHz: speech, the digit 5 over 0.8 .. 1.2 s, 1100 Hz over 1.6 .. 2.4 s, a speech burst over 2.8 .. 4.2 s; mu-law bytes, one per frame"""
    r = 8000
    sp = lambda sec, seed: speech_like_pcm(sec, seed=seed, rate=r).astype(np.float64) / 32768.0      # noqa: E731
    sig = np.concatenate([sp(0.8, 4), D.tone("5", 3200, r), np.zeros(3200), TR.sine(1100, 6400, r), np.zeros(3200), sp(1.4, 6), np.zeros(6400)])
    sig = sig + TR.noise(len(sig), -55.0, 2)
    return IF.encode(TR.to_pcm(sig), "mulaw")


# ------------------------------------------------------------------ modes
def mode_plain(gm, feed, save=None):
    pcm = speech_like_pcm(4.0, seed=int(os.environ.get("SNAP_SEED", "12")))
    out = {}
    for name, cut in (("early", 8000 + 37), ("mid", 36800)):
        ref, bad, blob = three(gm, {}, pcm, int(feed), cut)
        out[name] = dict(ref=ref, bad=bad)
        if save and name == "mid":
            open(save, "wb").write(blob)
    g0 = gm.snapshot_stats(0)
    out["stats"] = list(g0[:2])
    return out


def mode_engine2(gm):
    pcm = speech_like_pcm(4.0, seed=12)
    ref, bad, _ = three(gm, {}, pcm, 1600, 36800)
    return dict(ref=ref, bad=bad, dev0=list(gm.snapshot_stats(0)[:2]), dev1=list(gm.snapshot_stats(1)[:2]))


def mode_proc_src(gm, path):
    pcm = speech_like_pcm(4.0, seed=12)
    cut = 56000
    s = Stream(gm)
    s.feed(pcm, bounds(0, cut, 1600))
    mark, rows_cut = len(s.log), s.rows_written()
    blob = s.s.snapshot()
    s.feed(pcm, bounds(cut, len(pcm), 1600)); s.s.flush()
    p = R.parse(blob)
    open(path, "wb").write(blob)
    json.dump(dict(after=s.log[mark:], end=s.state(), rows=digest(s.rows(rows_cut))), open(path + ".json", "w"))
    return dict(rows_written=rows_cut, ring=p["book"]["ring_frames"], avail=p["book"]["avail"], tail=p["book"]["tail"], head=p["book"]["head"])


def mode_proc_dst(gm, path):
    pcm = speech_like_pcm(4.0, seed=12)
    cut = 56000
    ref = uninterrupted(gm, {}, pcm, 1600, cut)
    src = json.load(open(path + ".json"))
    blob = open(path, "rb").read()
    bad = []
    t = Stream(gm)
    t.s.restore(blob)
    if t.state() != ref["at_cut"]:
        bad.append("restored state differs at the cut")
    t.feed(pcm, bounds(cut, len(pcm), 1600)); t.s.flush()
    compare("copy", ref, t, 0, bad)
    if src["after"] != ref["log"][ref["mark"]:] or src["end"] != json.loads(json.dumps(ref["end"])) or src["rows"] != ref["rows"]:
        bad.append("the source process went on differently from the uninterrupted run")
    ring = int(t.s._L.aprilx_session_read_frames(t.s._handle, 0, 0, None))
    return dict(bad=bad, finals_after=ref["finals_after"], partials_after=ref["partials_after"], rows_written=ring, info_ring=R.parse(blob)["book"]["ring_frames"])


def mode_all(gm):
    cfg, bias = all_cfg(gm)
    data = all_audio()
    out = {}
    for name, cut in (("digit", 8000), ("tone", 16000), ("speech", 28000 + 13)):
        ref, bad, blob = three(gm, cfg, data, 800, cut)
        out[name] = dict(ref=ref, bad=bad)
        log_kinds = ref["kinds_before"], ref["kinds_after"]
        out[name]["kinds"] = log_kinds
    i = A.snapshot_info(blob)
    want = dict(input_rate=8000, input_format=("mulaw", 1, 0), alternatives=4, search_options=(600, 0.5, 2000))
    info_bad = [k for k, v in want.items() if i[k] != v]
    if i["vad"] is None or i["vad"]["onset_ms"] != 40 or i["vad"]["hangover_ms"] != 300 or i["dtmf"] is None or i["dtmf"]["min_tone_ms"] != 20 or i["tones"] is None or i["tones"]["min_tone_ms"] != 80:
        info_bad.append("detectors")
    st, ed = C.c_int32(0), C.c_int64(0)
    gm._L.aprilx_bias_info(bias._handle, C.byref(st), C.byref(ed))
    if i["bias"] is None or (i["bias"]["states"], i["bias"]["edges"], i["bias"]["flags"]) != (st.value, ed.value, 0) or i["bias"]["hash"] == 0:
        info_bad.append("bias")
    if (i["sample_rate"], i["vocab"], i["precision"]) != (gm.dims.sample_rate, gm.dims.vocab, 0):
        info_bad.append("identity")
    out["info_bad"] = info_bad
    return out


def mode_edges(gm):
    pcm = speech_like_pcm(3.0, seed=12)
    out = {}
    for name, kw in (("never_fed", dict(cut=0)), ("after_flush", dict(cut=32000, flush_at_cut=True))):
        ref, bad, _ = three(gm, {}, pcm, 1600, **kw)
        out[name] = dict(ref=ref, bad=bad)
    pcm8 = speech_like_pcm(3.0, seed=12, rate=8000)
    ref, bad, blob = three(gm, dict(input_sample_rate=8000), pcm8, 800, 10400 + 5)
    out["resampled"] = dict(ref=ref, bad=bad, segs=len(R.parse(blob)["book"]["segs"]), in_rate=R.parse(blob)["book"]["rs_in_rate"])
    return out


def mode_contents(gm):
    pcm = speech_like_pcm(4.0, seed=12)
    cut = 36800
    s = Stream(gm)
    s.feed(pcm, bounds(0, cut, 1600))
    blob = s.s.snapshot()
    p, st = R.parse(blob), s.state()
    bad = []
    if p["search"]["ctx"] != st["ctx"]:
        bad.append("ctx")
    g = np.frombuffer(p["device"]["arrays"]["gstate"]["data"], np.int32).tolist()
    if g != st["dev"]:
        bad.append("device search state %r against %r" % (g, st["dev"]))
    if (p["session"]["chunks"], p["session"]["real_frames"], p["book"]["rows_written"]) != (st["chunks"], st["frames_seen"], st["rows_written"]):
        bad.append("counters")
    stride = gm.dims.frame_shift * 1000 // gm.dims.sample_rate * int(p["book"]["seg_step"])
    if p["session"]["now_ms"] != st["chunks"] * stride or p["info"]["now_ms"] != p["session"]["now_ms"]:
        bad.append("now_ms %d with %d chunks of %d ms" % (p["session"]["now_ms"], st["chunks"], stride))
    avail = p["book"]["avail"]
    if not (0 < avail < p["book"]["seg_count"]) or p["device"]["ring_rows"] != avail:
        bad.append("avail %d" % avail)
    if not np.array_equal(p["device"]["ring"].view(np.uint32), s.rows(st["rows_written"] - avail, avail).view(np.uint32)):
        bad.append("ring rows")
    tail = np.frombuffer(p["book"]["audio"], "<i2")
    consumed = st["frames_seen"] * gm.dims.frame_shift
    if p["book"]["fifo_pos"] != 0 or not np.array_equal(tail, pcm[consumed:cut]) or len(tail) == 0:
        bad.append("audio tail: %d samples, %d expected" % (len(tail), cut - consumed))
    if p["info"]["ring_rows"] != avail or p["info"]["chunks"] != st["chunks"] or p["info"]["vocab"] != gm.dims.vocab or p["info"]["n_layers"] != gm.dims.n_layers:
        bad.append("info")
    h = np.frombuffer(p["device"]["arrays"]["h"]["data"], np.float32)
    if not np.isfinite(h).all() or not np.any(h != 0):
        bad.append("h rows are zero or not finite")
    s.s.close()
    return dict(bad=bad, avail=avail, tail=len(tail), blob_bytes=len(blob), device_bytes=p["device"]["bytes"])


def mode_batched(gm, n):
    n = int(n)
    pcms = [speech_like_pcm(2.0, seed=100 + i) for i in range(n)]
    cut, feed = 16000 + 17, 1600

    def run(migrate):
        logs = [[] for _ in range(n)]

        def make():
            ss = [A.Session(gm, (lambda t, toks, i=i: logs[i].append([int(t), [[k[0], bits(k[1]), k[2], k[3]] for k in toks]])), raw_events=True) for i in range(n)]
            return ss, A.SessionGroup(ss)
        ss, g = make()
        for a, b in bounds(0, cut, feed):
            g.feed([p[a:b] for p in pcms])
        counts = None
        if migrate:
            before = gm.snapshot_stats(0)
            blobs = g.snapshot()
            mid = gm.snapshot_stats(0)
            for s in ss:
                s.close()
            ss, g = make()
            g.restore(blobs)
            after = gm.snapshot_stats(0)
            counts = dict(gathers=mid[0] - before[0], scatters=after[1] - mid[1], other=(mid[1] - before[1]) + (after[0] - mid[0]), bytes=sum(len(b) for b in blobs))
        for a, b in bounds(cut, len(pcms[0]), feed):
            g.feed([p[a:b] for p in pcms])
        g.flush()
        chunks = [s.chunks() for s in ss]
        for s in ss:
            s.close()
        return hashlib.sha1(repr(logs).encode()).hexdigest(), sum(len(x) for x in logs), len({repr(x) for x in logs}), chunks, counts
    d0, n0, distinct, c0, _ = run(False)
    d1, n1, _, c1, counts = run(True)
    return dict(same=d0 == d1 and c0 == c1, callbacks=n0, callbacks_migrated=n1, distinct=distinct, counts=counts, mismatch=gm.stats().replay_mismatch)


def normal_stream(gm, stream, cfg, data, feed):
    """`stream` (fresh, or what a refusal left) over the whole audio against a session created for it: must be the same"""
    u = Stream(gm, **cfg)
    for x in (u, stream):
        x.feed(data, bounds(0, len(data), feed)); x.s.flush()
    same = u.log == stream.log and u.state() == stream.state() and len(u.log) > 0
    u.s.close()
    return same


def mode_refusals(gm, other_path):
    cfg, bias = all_cfg(gm)
    data = all_audio()
    src = Stream(gm, **cfg)
    src.feed(data, bounds(0, 16000, 800))
    blob = src.s.snapshot()
    out = {}

    def refused(stream, b=blob):
        try:
            stream.s.restore(b)
        except ValueError as e:
            return str(e)
        return None
    # one field at a time
    other_bias = gm.bias(session_phrases(model_texts(gm), gm.dims.blank_id, np.random.default_rng(4)))
    changes = dict(rate=dict(input_sample_rate=11025), format=dict(input_format="alaw"), no_format=dict(input_format=None), k=dict(alternatives=3), no_k=dict(alternatives=None),
                   endpoint=dict(endpoint_silence_ms=700), penalty=dict(blank_penalty=0.25), max_utt=dict(max_utterance_ms=3000), vad=dict(vad=dict(onset_ms=50)),
                   no_vad=dict(vad=None), no_dtmf=dict(dtmf=None), dtmf=dict(dtmf=dict(min_share=0.5)), tones=dict(tones=True), no_tones=dict(tones=None),
                   no_bias=dict(bias=None), other_bias=dict(bias=other_bias))
    msgs, usable = {}, {}
    for name, ch in changes.items():
        c2 = dict(cfg, **ch)
        t = Stream(gm, **c2)
        msgs[name] = refused(t)
        if name in ("rate", "no_format", "no_bias", "k"):
            d = data if c2.get("input_format") else speech_like_pcm(1.0, seed=3, rate=8000)
            usable[name] = normal_stream(gm, t, c2, d[:8000], 800)
        t.s.close()
    out["config"], out["config_usable"] = msgs, usable
    # a corrupt blob, a blob of another model, a target that has been fed: the same target, which then runs a normal stream
    t = Stream(gm, **cfg)
    flipped = bytearray(blob); flipped[len(blob) // 2] ^= 4
    out["corrupt"] = [refused(t, bytes(flipped)), refused(t, blob[:-1]), refused(t, b"")]
    om = A.Model(other_path)
    o = Stream(om)
    o.feed(speech_like_pcm(0.5, seed=1, rate=8000), [(0, 4000)])
    out["other_model"] = refused(t, o.s.snapshot())
    plain = Stream(gm)
    plain.feed(speech_like_pcm(0.5, seed=1), [(0, 8000)])
    out["other_config_blob"] = refused(t, plain.s.snapshot())
    out["target_usable"] = normal_stream(gm, t, cfg, data, 800)
    out["fed"] = refused(t)                                    # (flushed: it has chunks and rows behind it)
    t2 = Stream(gm, **cfg)
    t2.feed(data, [(0, 800)])
    out["fed_open"] = refused(t2)
    t2.s.close()
    # the accepted case, as the control of all of the above
    t3 = Stream(gm, **cfg)
    out["control"] = refused(t3)
    t3.s.close()
    # cap too small
    L = gm._L
    need = int(L.aprilx_session_snapshot(src.s._handle, None, 0))
    buf = (C.c_char * need)()
    out["cap"] = [int(L.aprilx_session_snapshot(src.s._handle, C.addressof(buf), need - 1)), int(L.aprilx_session_snapshot(src.s._handle, C.addressof(buf), need)) == need]
    # from the session's own handler: synchronous (the caller's thread) and asynchronous (the stepping thread)
    for kind in ("sync", "async"):
        h = Stream(gm, asynchronous=kind == "async")
        got = []
        h.hook = lambda h=h, got=got: got.append(int(L.aprilx_session_snapshot(h.s._handle, None, 0)))
        pcm = speech_like_pcm(2.0, seed=12)
        h.feed(pcm, bounds(0, len(pcm), 1600))
        h.s.drain()
        h.hook = None
        out["handler_" + kind] = [len(got), sorted(set(got))]
        out["handler_%s_after" % kind] = int(L.aprilx_session_snapshot(h.s._handle, None, 0)) > 0
        h.s.flush(); h.s.close()
    src.feed(data, bounds(16000, len(data), 800)); src.s.flush()
    out["source_events"] = len(src.log)
    return out


def mode_refuse_file(gm, path):
    t = Stream(gm)
    try:
        t.s.restore(open(path, "rb").read())
        msg = None
    except ValueError as e:
        msg = str(e)
    pcm = speech_like_pcm(1.0, seed=12)
    return dict(msg=msg, usable=normal_stream(gm, t, {}, pcm, 1600))


def mode_scan(gm, lo, hi):
    """per seed: (PARTIALs, FINALs, most active tokens) delivered after 0.5 s, 2.3 s and 3.5 s of speech_like_pcm(4 s) -- how the seeds of the tests were picked"""
    out = {}
    for seed in range(int(lo), int(hi)):
        pcm = speech_like_pcm(4.0, seed=seed)
        u = Stream(gm)
        marks = {}
        for a, b in bounds(0, len(pcm), 1600):
            if a in (8000, 36800, 56000):
                marks[a] = len(u.log)
            u.s.feed(pcm[a:b])
        u.s.flush()
        out[seed] = [[count(u.log[m:], PARTIAL), count(u.log[m:], FINAL), max([len(e[2]) for e in u.log[m:]] or [0])] for m in marks.values()]
        u.s.close()
    return out


if __name__ == "__main__":
    gm = A.Model(sys.argv[1])
    res = globals()["mode_" + sys.argv[2]](gm, *sys.argv[3:])
    print("RESULT " + json.dumps(res))
    gm.close()
