"""april_asr_amd/csrc/gemm_kw_asm.inc is generated code: it must be what tools/gen_kw_asm.py prints (the generator also checks its
own wait counts: every replay of the instruction stream must ask the same vmcnt of a wait)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kw_asm_inc_is_current():
    want = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "gen_kw_asm.py")]).decode()
    with open(os.path.join(ROOT, "april_asr_amd", "csrc", "gemm_kw_asm.inc")) as f:
        have = f.read()
    assert have == want, "regenerate: python tools/gen_kw_asm.py > april_asr_amd/csrc/gemm_kw_asm.inc"
