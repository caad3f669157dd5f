"""The queue between the client threads and the stepping thread of the per-slot opt-in tables (csrc/slot_queue.h; DESIGN.md section 12,
"life cycle") as a stand-alone program (tests/cpp/slot_queue_test.cc): four pushers and one taker on 8 slots, under
AddressSanitizer + UBSan and under ThreadSanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "april_asr_amd", "csrc")


@pytest.mark.parametrize("sanitizer", ["address,undefined", "thread"])
def test_queue_under_sanitizers(tmp_path, sanitizer):
    exe = str(tmp_path / "slot_queue_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", "-fsanitize=" + sanitizer, "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "slot_queue_test.cc"), "-o", exe], timeout=600)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0 and "all checks passed" in out, out[-3000:]
