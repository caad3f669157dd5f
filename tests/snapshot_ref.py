"""The snapshot blob stated independently of the library, with `struct` alone: build() puts a blob together from
plain values, parse() takes one apart.  tests/test_snapshot_cpu.py feeds build()'s blobs to aprilx_snapshot_info;
tests/snapshot_worker.py reads the library's blobs with parse() and compares what they hold with the session's own getters.

Everything is little-endian.
  header (128 bytes)   "APXSNAP1", u32 version = 1, u32 blocks = 5, u64 total size, 5 x (u64 offset, u64 length), 3 x u64 0
  blocks               info, search, book, session, device -- in this order, each at an 8-byte aligned offset, zero padded
  trailer              u64 FNV-1a 64 of every byte before it
"""
import struct

import numpy as np

MAGIC = b"APXSNAP1"
VERSION = 1
HEADER = 128
BLOCKS = ("info", "search", "book", "session", "device")

# the info block: AprilxSnapshotInfo, 512 bytes
INFO_FIELDS = (["size", "version", "blob_size", "params_hash", "token_hash", "bias_hash", "bias_edges", "chunks", "frames_seen", "now_ms", "rows_written"]
               + ["n_layers", "d_model", "hidden", "ffn", "joiner", "vocab", "mel", "segment_size", "segment_step", "sample_rate", "frame_shift_ms", "blank_id"]
               + ["precision", "f16_tile", "input_rate", "confidence_k", "has_format", "has_search_options", "has_vad", "has_dtmf", "has_tones", "has_bias", "bias_flags"]
               + ["bias_states", "ring_rows", "reserved"])
INFO_HEAD = "<IIQQQQqQQQQ" + "12i" + "11I" + "iII"
FORMAT = ("<IIIi", ("size", "encoding", "channels", "channel"))
SEARCH = ("<IIIf", ("size", "endpoint_silence_ms", "max_utterance_ms", "blank_penalty"))
VAD = ("<IffffIIfI", ("size", "band_lo_hz", "band_hi_hz", "onset_db", "offset_db", "onset_ms", "hangover_ms", "min_energy", "flags"))
DTMF = ("<IfffffIII", ("size", "min_level_dbfs", "twist_hi_db", "twist_lo_db", "rel_peak_db", "min_share", "min_tone_ms", "min_pause_ms", "flags"))
TONES = ("<IfffIIII", ("size", "min_level_dbfs", "second_db", "min_share", "tol_hz", "min_tone_ms", "min_pause_ms", "flags"))
SUBS = (("format", FORMAT), ("search", SEARCH), ("vad", VAD), ("dtmf", DTMF), ("tones", TONES))
INFO_BYTES = 512
assert struct.calcsize(INFO_HEAD) + sum(struct.calcsize(f) for _, (f, _n) in SUBS) + 64 + 128 == INFO_BYTES

DEVICE_ARRAYS = ("h", "c", "h16", "eout", "dout", "gstate", "bias_state", "vad_state", "ring")


def fnv1a(data: bytes) -> int:
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def pack_info(info: dict) -> bytes:
    out = struct.pack(INFO_HEAD, *[info.get(n, 0) for n in INFO_FIELDS])
    for name, (fmt, fields) in SUBS:
        sub = info.get(name) or {}
        out += struct.pack(fmt, *[sub.get(n, 0) for n in fields])
    out += struct.pack("<64s128s", info.get("name", b""), info.get("description", b""))
    assert len(out) == INFO_BYTES
    return out


def unpack_info(b: bytes) -> dict:
    n = struct.calcsize(INFO_HEAD)
    info = dict(zip(INFO_FIELDS, struct.unpack(INFO_HEAD, b[:n])))
    for name, (fmt, fields) in SUBS:
        k = struct.calcsize(fmt)
        info[name] = dict(zip(fields, struct.unpack(fmt, b[n:n + k])))
        n += k
    info["name"], info["description"] = (x.rstrip(b"\0") for x in struct.unpack("<64s128s", b[n:n + 192]))
    return info


def example_info() -> dict:
    """an info block with every field different from every other, for the tests that read it back"""
    info = {n: 1000 + i for i, n in enumerate(INFO_FIELDS)}
    info.update(size=INFO_BYTES, version=VERSION, reserved=0, bias_edges=-7, blank_id=-3, has_format=1, has_search_options=1, has_vad=1, has_dtmf=0, has_tones=1, has_bias=1)
    info["format"] = dict(size=16, encoding=1, channels=2, channel=-1)
    info["search"] = dict(size=16, endpoint_silence_ms=700, max_utterance_ms=5000, blank_penalty=0.25)
    info["vad"] = dict(size=36, band_lo_hz=300.0, band_hi_hz=3400.0, onset_db=6.0, offset_db=2.5, onset_ms=40, hangover_ms=200, min_energy=-11.0, flags=0)
    info["dtmf"] = dict(size=0)
    info["tones"] = dict(size=32, min_level_dbfs=-35.0, second_db=12.0, min_share=0.5, tol_hz=25, min_tone_ms=80, min_pause_ms=40, flags=0)
    info["name"], info["description"] = b"a model", b"its description"
    return info


def build(info: dict, search=b"", book=b"", session=b"", device=b"", magic=MAGIC, version=VERSION, size=None, blocks=5) -> bytes:
    """a whole blob; info["blob_size"] and the header's size are the real total unless `size` overrides the header's"""
    parts = [None, search, book, session, device]
    lens = [INFO_BYTES] + [len(p) for p in parts[1:]]
    total = HEADER + sum((n + 7) // 8 * 8 for n in lens) + 8
    info = dict(info, blob_size=total)
    parts[0] = pack_info(info)
    head = magic + struct.pack("<IIQ", version, blocks, total if size is None else size)
    at = HEADER
    for n in lens:
        head += struct.pack("<QQ", at, n)
        at += (n + 7) // 8 * 8
    head += struct.pack("<QQQ", 0, 0, 0)
    assert len(head) == HEADER
    body = b"".join(p + b"\0" * (-len(p) % 8) for p in parts)
    blob = head + body
    return blob + struct.pack("<Q", fnv1a(blob))


def parse(blob: bytes) -> dict:
    """the blob's contents as plain values; AssertionError where it does not follow the format"""
    assert blob[:8] == MAGIC
    version, nblk, total = struct.unpack("<IIQ", blob[8:24])
    assert (version, nblk, total) == (VERSION, 5, len(blob))
    assert struct.unpack("<Q", blob[-8:])[0] == fnv1a(blob[:-8])
    raw = {}
    for i, name in enumerate(BLOCKS):
        off, n = struct.unpack("<QQ", blob[24 + 16 * i:40 + 16 * i])
        assert off % 8 == 0 and off + n <= len(blob) - 8
        raw[name] = blob[off:off + n]
    out = {"info": unpack_info(raw["info"])}
    assert out["info"]["blob_size"] == len(blob)
    # search state: ctx[2], trie state, K, evals, head, last_call_head, last_emit_ms, first_ms, emitted_silence, entry count; then the entries
    g = raw["search"]
    f = struct.unpack("<iiiIQQQQQII", g[:64])
    s = dict(ctx=[f[0], f[1]], bias_state=f[2], conf_k=f[3], evals=f[4], head=f[5], last_call_head=f[6], last_emit_ms=f[7], first_ms=f[8], emitted_silence=f[9])
    s["tokens"] = [dict(zip(("id", "logprob", "flags", "time_ms"), (t[0], t[1], t[2], t[4]))) for t in struct.iter_unpack("<ifIIQ", g[64:64 + 24 * f[10]])]
    s["infos"] = [g[64 + 24 * f[10] + 96 * i:64 + 24 * f[10] + 96 * (i + 1)] for i in range(f[10] if f[3] else 0)]
    assert len(g) == 64 + (24 + (96 if f[3] else 0)) * f[10]
    out["search"] = s
    # frame book
    b = raw["book"]
    f = struct.unpack("<8iqqQQqqIIIIiIIIQ", b[:120])
    k = dict(zip(("shift", "padded", "seg_count", "seg_step", "ring_frames", "head", "tail"), f[:7]))
    k.update(zip(("avail", "avail_shadow", "rows_written", "fifo_pos", "in_drop", "rs_end", "rs_in_rate", "rs_out_rate"), f[8:16]))
    k["format"] = dict(encoding=f[16], channels=f[17], channel=f[18], frame_bytes=f[19])
    nseg, abytes = f[20], f[22]
    k["segs"] = [dict(zip(("pos", "in_start", "n_in", "n_out", "zeros", "closed"), t)) for t in struct.iter_unpack("<qqqqqQ", b[120:120 + 48 * nseg])]
    k["audio"] = b[120 + 48 * nseg:120 + 48 * nseg + abytes]
    assert len(b) == 120 + 48 * nseg + abytes
    out["book"] = k
    # session
    q = raw["session"]
    assert len(q) == 120
    fl = q[:8]
    f = struct.unpack("<QQQQIiiiiIQQiiiiiiQQ", q[8:])
    out["session"] = dict(dout_ready=fl[0], was_flushed=fl[1], seg_open=fl[2], vad_on=fl[3], vad_reset=fl[4], dtmf_on=fl[5], tones_on=fl[6],
                          now_ms=f[0], chunks=f[1], real_frames=f[2], vad_speech=f[3], vad_segments=f[4], vad_last=f[5],
                          dtmf=dict(held=f[6], cand=f[7], run=f[8], tone=f[10], digits=f[11]),
                          tones=dict(held=f[12], h1=f[13], h2=f[14], c1=f[15], c2=f[16], run=f[17], tonal=f[18], tones=f[19]))
    # device block: array count, ring rows, mask, block bytes; per array (rows, row bytes, offset, 0); the block
    d = raw["device"]
    na, rows, mask, nbytes = struct.unpack("<IIII", d[:16])
    assert na == len(DEVICE_ARRAYS) and len(d) == 16 + 16 * na + nbytes
    block = d[16 + 16 * na:]
    dev = dict(ring_rows=rows, mask=mask, bytes=nbytes, arrays={})
    for i, name in enumerate(DEVICE_ARRAYS):
        layers, row_bytes, off, z = struct.unpack("<IIII", d[16 + 16 * i:32 + 16 * i])
        assert z == 0 and off % 16 == 0
        n = rows if name == "ring" else layers
        dev["arrays"][name] = dict(rows=n, row_bytes=row_bytes, off=off, data=block[off:off + n * row_bytes])
    r = dev["arrays"]["ring"]
    dev["ring"] = np.frombuffer(r["data"], np.float32).reshape(rows, r["row_bytes"] // 4) if rows else np.zeros((0, r["row_bytes"] // 4), np.float32)
    out["device"] = dev
    return out
