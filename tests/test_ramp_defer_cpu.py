"""The host's bookkeeping of a deferred layer graph (csrc/ramp_defer.h; DESIGN.md section 4.2, "deferred enqueue") as a stand-alone
program (tests/cpp/ramp_defer_test.cc): scripted orders of launches, polls and outcome words -- hosted before the poll, not hosted,
settled by another entry, no hosting chain in front, two feeds in a row, a stale generation in the word -- built plain and under
AddressSanitizer + UBSan (a host program: it never touches a GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "april_asr_amd", "csrc")


@pytest.mark.parametrize("sanitizer", ["", "address,undefined"])
def test_ramp_defer_state_machine(tmp_path, sanitizer):
    exe = str(tmp_path / "ramp_defer_test")
    flags = ["-fsanitize=" + sanitizer, "-fno-sanitize-recover=all"] if sanitizer else []
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + flags +
                          ["-I", CSRC, os.path.join(ROOT, "tests", "cpp", "ramp_defer_test.cc"), "-o", exe], timeout=600)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0 and "all checks passed" in out, out[-3000:]
