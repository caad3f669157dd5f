"""Session snapshots without a GPU: the blob's container and its info block, built by the independent statement
of the layout (tests/snapshot_ref.py) and read by aprilx_snapshot_info; every truncation, seeded single-byte flips, a wrong magic,
version and size; and csrc/snapshot.h alone under AddressSanitizer + UBSan as a stand-alone program (tests/cpp/snapshot_test.cc)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import april_asr_amd as A
from april_asr_amd import _ffi
import snapshot_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "april_asr_amd", "csrc")


def info_rc(blob):
    out = _ffi.AprilxSnapshotInfo()
    return _ffi.lib().aprilx_snapshot_info(bytes(blob), len(blob), C.byref(out)), out


def test_info_returns_the_stored_fields(built):
    want = R.example_info()
    blob = R.build(want, search=b"\1" * 13, book=b"\2" * 8, session=b"", device=b"\3" * 100)
    rc, got = info_rc(blob)
    assert rc == 0
    assert C.sizeof(_ffi.AprilxSnapshotInfo) == R.INFO_BYTES
    for n in R.INFO_FIELDS:
        assert getattr(got, n) == (len(blob) if n == "blob_size" else want[n]), n
    for name, (_fmt, fields) in R.SUBS:
        for n in fields:
            assert getattr(getattr(got, name), n) == want[name].get(n, 0), (name, n)
    assert got.name == want["name"] and got.description == want["description"]
    d = A.snapshot_info(blob)
    assert d["input_format"] == ("mulaw", 2, -1) and d["search_options"] == (700, 0.25, 5000) and d["dtmf"] is None
    assert d["vad"]["hangover_ms"] == 200 and d["tones"]["tol_hz"] == 25 and d["bias"]["edges"] == -7
    assert d["alternatives"] == want["confidence_k"] and d["input_rate"] == want["input_rate"] and d["name"] == "a model"
    # the reference's own parser reads its own blob back
    assert R.unpack_info(blob[R.HEADER:R.HEADER + R.INFO_BYTES])["vad"]["onset_ms"] == 40


def test_every_truncation_is_refused(built):
    blob = R.build(R.example_info(), search=b"\5" * 24, device=b"\7" * 64)
    assert info_rc(blob)[0] == 0
    for n in range(len(blob)):                       # the header, and everything behind it
        assert info_rc(blob[:n])[0] == -1, n
    assert info_rc(blob + b"\0")[0] == -1
    assert _ffi.lib().aprilx_snapshot_info(None, 0, C.byref(_ffi.AprilxSnapshotInfo())) == -1
    assert _ffi.lib().aprilx_snapshot_info(blob, len(blob), None) == -1


def test_single_byte_flips_are_refused(built):
    blob = bytearray(R.build(R.example_info(), search=b"\5" * 24, book=b"\6" * 40, session=b"\1" * 16, device=b"\7" * 200))
    rng = np.random.RandomState(19)
    pos = sorted(set(rng.randint(0, len(blob), size=400).tolist()))[:200]
    assert len(pos) == 200
    for p in pos:
        bad = bytearray(blob)
        bad[p] ^= 1 << int(rng.randint(0, 8))
        assert info_rc(bad)[0] == -1, p


def test_wrong_magic_version_and_size_are_refused(built):
    """each with the hash computed over the blob as it is, so that it is the field that is refused"""
    info = R.example_info()
    assert info_rc(R.build(info))[0] == 0
    assert info_rc(R.build(info, magic=b"APXSNAP2"))[0] == -1
    assert info_rc(R.build(info, magic=b"\0" * 8))[0] == -1
    assert info_rc(R.build(info, version=0))[0] == -1
    assert info_rc(R.build(info, version=2))[0] == -1
    good = R.build(info)
    for size in (0, len(good) - 8, len(good) + 8, 2 ** 63):
        assert info_rc(R.build(info, size=size))[0] == -1, size
    assert info_rc(R.build(info, blocks=4))[0] == -1
    # an info block that disagrees with the header about the size, or is of another version
    bad = bytearray(good)
    bad[R.HEADER + 8:R.HEADER + 16] = struct.pack("<Q", len(good) + 1)
    bad[-8:] = struct.pack("<Q", R.fnv1a(bytes(bad[:-8])))
    assert info_rc(bad)[0] == -1
    assert info_rc(R.build(dict(info, version=2)))[0] == -1


def test_header_alone_under_sanitizers(built, tmp_path):
    """csrc/snapshot.h: Greedy, FrameBook (plain, resampled, formatted with a raw tail) and the detectors' machines round trip field by
    field, and the parser refuses the same corrupt inputs; AddressSanitizer + UBSan, stand-alone (session.cc is compiled in for the state
    machine the images are taken from; no engine is linked)"""
    exe = str(tmp_path / "snapshot_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-result", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "snapshot_test.cc"),
                           os.path.join(CSRC, "session.cc"), os.path.join(ROOT, "tests", "sched_harness", "fake_engine.cc"), "-o", exe, "-lpthread"], timeout=600)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0 and "all checks passed" in out, out[-3000:]
