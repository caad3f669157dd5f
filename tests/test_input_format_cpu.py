"""Input formats without a GPU: the contract in plain C++ (aprilx_decode_host) against its numpy statement
(tests/input_format_ref.py), every comparison exact; and the host decode plus the raw-byte queue of a formatted session under
AddressSanitizer + UBSan as a stand-alone program (tests/cpp/input_format_test.cc)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import april_asr_amd as A
from april_asr_amd import _ffi
import input_format_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "april_asr_amd", "csrc")


def host(data, enc, channels=1, channel=0):
    return A.decode_host(data, (enc, channels, channel))


def f32_cases():
    rng = np.random.RandomState(15)
    edge = [p / 32768.0 for p, _ in R.F32_PRODUCTS] + [x for x, _ in R.F32_VALUES]
    ties = (rng.randint(-32770, 32770, size=1024) + 0.5) / 32768.0          # exact .5 ties, some past the clamp
    near = rng.randint(-40000, 40000, size=1024) / 32768.0 + rng.uniform(-1e-5, 1e-5, size=1024)
    wide = rng.uniform(-1.2, 1.2, size=1024)
    bits = rng.randint(0, 2 ** 32, size=1024, dtype=np.uint64).astype(np.uint32).view(np.float32)      # any bit pattern: NaNs, infinities, denormals
    return np.concatenate([np.array(edge, np.float32), ties.astype(np.float32), near.astype(np.float32), wide.astype(np.float32), bits])


def test_literal_values_of_the_contract(built):
    for enc, code, want in R.LITERALS:
        assert int(host(bytes([code]), enc)[0]) == want == int(R.decode(bytes([code]), enc)[0]), (enc, hex(code))
    for prod, want in R.F32_PRODUCTS:
        x = np.array([prod / 32768.0], np.float32)
        assert int(host(x, "f32")[0]) == want == int(R.decode(x, "f32")[0]), prod
    for x, want in R.F32_VALUES:
        a = np.array([x], np.float32)
        assert int(host(a, "f32")[0]) == want == int(R.decode(a, "f32")[0]), x


def test_all_256_codes_of_both_laws(built):
    codes = np.arange(256, dtype=np.uint8)
    for enc in ("mulaw", "alaw"):
        got = host(codes, enc)
        assert got.dtype == np.int16 and (got == R.decode(codes, enc)).all()
        assert sorted(set(np.abs(got.astype(int)))) == sorted(set(np.abs(R.decode(codes, enc).astype(int))))
    # the laws are odd: code b and b ^ 0x80 decode to opposite values
    for enc in ("mulaw", "alaw"):
        v = host(codes, enc).astype(int)
        assert (v == -v[codes ^ 0x80]).all()


def test_f32_edges_ties_and_random_bits(built):
    x = f32_cases()
    assert x.size >= 4096
    assert (host(x, "f32") == R.decode(x, "f32")).all()


@pytest.mark.parametrize("channels", [1, 2, 3, 8])
@pytest.mark.parametrize("enc", R.ENCODINGS)
def test_channels_and_lengths(built, enc, channels):
    rng = np.random.RandomState(channels * 7 + R.ENCODINGS.index(enc))
    for frames in (0, 1, 257):
        n = frames * channels
        if enc == "s16":
            raw = rng.randint(-32768, 32768, size=n).astype("<i2")
        elif enc == "f32":
            raw = f32_cases()[rng.randint(0, 4096, size=n)]
        else:
            raw = rng.randint(0, 256, size=n).astype(np.uint8)
        for channel in sorted({-1, 0, channels - 1}):
            got = host(raw, enc, channels, channel)
            assert got.size == frames and (got == R.decode(raw, enc, channels, channel)).all(), (enc, channels, channel, frames)


def test_downmix_extremes_and_ties(built):
    for c in (1, 2, 3, 8):
        assert (host(np.full(c * 3, -32768, "<i2"), "s16", c, -1) == -32768).all()
        assert (host(np.full(c * 3, 32767, "<i2"), "s16", c, -1) == 32767).all()
        assert (host(np.full(c, 4.0, np.float32), "f32", c, -1) == 32767).all() and (host(np.full(c, -4.0, np.float32), "f32", c, -1) == -32768).all()
    # C = 2: S = 1 -> 1, S = -1 -> 0, S = -3 -> -1 (half towards +infinity, the division floors)
    x = np.array([1, 0, -1, 0, -3, 0, 3, 0, -2, -1, 32767, 32766, -32768, -32767], "<i2")
    assert host(x, "s16", 2, -1).tolist() == [1, 0, -1, 2, -1, 32767, -32767] == R.decode(x, "s16", 2, -1).tolist()
    # ties of both signs at every channel count: S = +-C/2 (even C), and the neighbours of every multiple of C
    for c in (2, 3, 8):
        rows = []
        for s in list(range(-3 * c, 3 * c + 1)):
            row = np.zeros(c, np.int64); row[0] = s
            rows.append(row)
        x = np.array(rows).reshape(-1).astype("<i2")
        got = host(x, "s16", c, -1)
        assert (got == R.decode(x, "s16", c, -1)).all()
        assert got.tolist() == [int(np.floor(s / c + 0.5)) for s in range(-3 * c, 3 * c + 1)]


def test_refusals(built):
    L = _ffi.lib()
    out = np.zeros(16, np.int16)
    data = np.zeros(64, np.uint8)

    def call(enc, ch, c, nbytes, cap, size=None):
        f = _ffi.AprilxInputFormat(C.sizeof(_ffi.AprilxInputFormat) if size is None else size, enc, ch, c)
        return int(L.aprilx_decode_host(C.byref(f), data.ctypes.data, nbytes, out.ctypes.data, cap))
    assert call(0, 1, 0, 8, 16) == 4
    assert call(0, 1, 0, 7, 16) == -1                      # a partial frame
    assert call(3, 3, 0, 16, 16) == -1 and call(3, 3, 0, 24, 16) == 2
    assert call(1, 3, -1, 4, 16) == -1 and call(1, 3, -1, 6, 16) == 2
    assert call(1, 1, 0, 17, 16) == -1 and call(1, 1, 0, 16, 16) == 16      # a too-small cap
    assert call(0, 1, 0, 0, 0) == 0
    assert call(4, 1, 0, 4, 16) == -1 and call(0, 0, 0, 4, 16) == -1 and call(0, 9, 0, 36, 16) == -1
    assert call(0, 2, 2, 4, 16) == -1 and call(0, 2, -2, 4, 16) == -1
    assert call(0, 1, 0, 8, 16, size=12) == -1
    assert int(L.aprilx_decode_host(None, data.ctypes.data, 8, out.ctypes.data, 16)) == -1


def test_encoders_of_the_tests_round_trip(built):
    """the encoders the GPU tests make their input with, through the product's host decode: G.711 codes decode to the nearest
    representable value, F32 and S16 exactly; and Session.feed's byte view refuses what it does not name"""
    for bad in ([1, 2, 3], np.zeros(4, np.float64), np.zeros(4, np.int32)):
        with pytest.raises(TypeError):
            A.decode_host(bad, ("s16", 1, 0))
    x = np.random.RandomState(3).randint(-32768, 32768, size=4000).astype(np.int16)
    assert (host(R.encode(x, "s16"), "s16") == x).all() and (host(R.encode(x, "f32"), "f32") == x).all()
    for enc, table in (("mulaw", R.mulaw_table()), ("alaw", R.alaw_table())):
        y = host(R.encode(x, enc), enc).astype(int)
        assert (y == R.decode(R.encode(x, enc), enc)).all()
        best = np.abs(table[None, :] - x[:, None].astype(int)).min(axis=1)
        assert (np.abs(y - x) == best).all()


def test_host_decode_and_raw_queue_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "input_format_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "input_format_test.cc"), "-o", exe], timeout=600)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0 and "all checks passed" in out, out[-3000:]
