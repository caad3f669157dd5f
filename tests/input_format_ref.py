"""The input-format contract stated in numpy, from its rules and not from the product's code: what a session
with a format must decode its bytes to.  Also the encoders the tests use to make such bytes from int16 PCM.

  s16    little-endian int16, identity
  mulaw  u = ~b & 0xFF; mag = ((((u & 15) << 3) + 0x84) << ((u >> 4) & 7)) - 0x84; value = -mag when u & 0x80 else mag
  alaw   a = b ^ 0x55; e = (a >> 4) & 7; m = a & 15; mag = (m << 4) + 8 when e == 0 else ((m << 4) + 0x108) << (e - 1);
         value = mag when a & 0x80 else -mag
  f32    little-endian binary32: y = x * 32768 in fp32, NaN -> 0, clamp to [-32768, 32767], round half to even
  channel c >= 0 takes that channel; -1 is floor((2 S + C) / (2 C)) of the sum S of the frame's decoded values"""
import numpy as np

ENCODINGS = ("s16", "mulaw", "alaw", "f32")
BYTES = {"s16": 2, "mulaw": 1, "alaw": 1, "f32": 4}

# the literal values of the contract: (encoding, input, value)
LITERALS = [("mulaw", 0xFF, 0), ("mulaw", 0x7F, 0), ("mulaw", 0x00, -32124), ("mulaw", 0x80, 32124),
            ("alaw", 0xD5, 8), ("alaw", 0x55, -8), ("alaw", 0x2A, -32256), ("alaw", 0xAA, 32256)]
# F32: (x * 32768 written as the product, value) and (x, value)
F32_PRODUCTS = [(0.5, 0), (1.5, 2), (2.5, 2), (-1.5, -2)]
F32_VALUES = [(1.0, 32767), (-1.0, -32768), (np.inf, 32767), (-np.inf, -32768), (-0.0, 0), (1e-40, 0), (-1e-45, 0), (np.nan, 0)]


def mulaw_table():
    u = (~np.arange(256)) & 0xFF
    mag = ((((u & 15) << 3) + 0x84) << ((u >> 4) & 7)) - 0x84
    return np.where(u & 0x80, -mag, mag).astype(np.int64)


def alaw_table():
    a = np.arange(256) ^ 0x55
    e, m = (a >> 4) & 7, a & 15
    mag = np.where(e == 0, (m << 4) + 8, ((m << 4) + 0x108) << np.maximum(e - 1, 0))
    return np.where(a & 0x80, mag, -mag).astype(np.int64)


def f32_values(x):
    """float32 array -> int64 values by the F32 rule"""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        y = (x * np.float32(32768.0)).astype(np.float32)          # fp32 product
        y = np.where(np.isnan(y), np.float32(0), y)
        y = np.clip(y, np.float32(-32768.0), np.float32(32767.0))
        return np.rint(y).astype(np.int64)                        # rint: half to even


def values(data, encoding):
    """raw bytes -> every value, in order, as int64"""
    raw = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    if encoding == "s16":
        return raw.view("<i2").astype(np.int64)
    if encoding == "mulaw":
        return mulaw_table()[raw]
    if encoding == "alaw":
        return alaw_table()[raw]
    if encoding == "f32":
        return f32_values(raw.view("<f4"))
    raise ValueError(encoding)


def decode(data, encoding, channels=1, channel=0):
    """raw bytes of whole frames -> int16, one per frame"""
    v = values(data, encoding).reshape(-1, channels)
    if channel >= 0:
        out = v[:, channel]
    else:
        out = (2 * v.sum(axis=1) + channels) // (2 * channels)      # (numpy's // floors)
    assert out.size == 0 or (out.min() >= -32768 and out.max() <= 32767)
    return out.astype(np.int16)


def encode(pcm, encoding):
    """int16 PCM -> one value per sample in `encoding` (an array whose bytes are the raw data): G.711 as the code whose value is
    nearest, F32 as pcm / 32768 (exact), S16 as is"""
    pcm = np.asarray(pcm, np.int16)
    if encoding == "s16":
        return pcm.astype("<i2")
    if encoding == "f32":
        return (pcm.astype(np.float32) / np.float32(32768.0)).astype("<f4")
    table = mulaw_table() if encoding == "mulaw" else alaw_table()
    order = np.argsort(table, kind="stable")
    sv = table[order]
    i = np.clip(np.searchsorted(sv, pcm.astype(np.int64)), 1, 255)
    pick = np.where(np.abs(sv[i - 1] - pcm) <= np.abs(sv[i] - pcm), i - 1, i)
    return order[pick].astype(np.uint8)


def interleave(chans):
    """equal-length per-channel value arrays of one dtype -> the interleaved raw bytes"""
    return np.stack(chans, axis=1).reshape(-1).view(np.uint8).copy()


def make_raw(pcm, encoding, channels, seed=0):
    """`channels` interleaved channels in `encoding`: channel c carries pcm scaled by a seeded factor and shifted by c samples, so
    that every channel and their downmix are different, plausible signals.  Returns the raw bytes (uint8 array)."""
    rng = np.random.RandomState(seed)
    chans = []
    for c in range(channels):
        g = 1.0 if c == 0 else float(rng.uniform(0.3, 0.9)) * (-1 if c % 2 else 1)
        x = np.roll(np.asarray(pcm, np.int16).astype(np.float64), 37 * c) * g
        chans.append(encode(np.clip(np.rint(x), -32768, 32767).astype(np.int16), encoding))
    return interleave(chans)
