"""The layout of the block a front-end pass's observers write (csrc/pass_layout.h) as a stand-alone program under AddressSanitizer +
UBSan (tests/cpp/pass_layout_test.cc): the parts' offsets and the block's length against the three formulas the function replaced
(FrontPass::quality_at_of, the head of Engine::fbank(), the tail of Scheduler::cut_frames()), frozen literally in the program, for every
combination of VAD and DTMF frames in {0, 1, 2, 3, 4, 5, 15, 16, 17, 1000} and tone and quality frames in {0, 1, 5}; alignment, no
overlap, and a block that ends with its last non-empty part."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "april_asr_amd", "csrc")


def test_layout_equals_the_three_formulas_it_replaced_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "pass_layout_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "pass_layout_test.cc"), "-o", exe], timeout=600)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0 and "all checks passed" in out, out[-3000:]
