"""The layout of Engine::fbank()'s staging buffer (csrc/staging_layout.h) as a stand-alone program under AddressSanitizer + UBSan
(tests/cpp/staging_layout_test.cc): offsets, upload length, regrow condition and capacities against the formulas the function replaced,
restated literally in the program, for all eight on/off combinations of the resample / decode / VAD passes; the DTMF array, which those
formulas did not know, against what the layout promises for it, and calls without it against the formulas unchanged."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "april_asr_amd", "csrc")


def test_layout_equals_the_formulas_it_replaced_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "staging_layout_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "staging_layout_test.cc"), "-o", exe], timeout=600)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0 and "all checks passed" in out, out[-3000:]
