"""The environment names the library reads and the table that documents them are one list: every "APRIL_..." string literal
under csrc/ has a row in the "Environment" table of INTEGRATION.md and every row names a literal that exists.  The names of
the forms that were built, measured and removed (LAB_NOTES.md) stay gone from the package, the tools, the tests and the
examples."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REMOVED = """APRIL_RECUR_KSPLIT APRIL_RECUR_KSPLIT_WGS APRIL_KW_GATES APRIL_KW_GATES_MAX_ROWS APRIL_KW_MIXED APRIL_KW_XCD APRIL_KW_SKEW
APRIL_KW_RING APRIL_GEMM_SKEW APRIL_SKEW_MIN_WGS APRIL_SKEW_SLOTS APRIL_TILE_NT6 APRIL_TILE_WIDE APRIL_TILE_BIG_NT APRIL_TILE_BIG_F32
APRIL_FF1_BALANCE APRIL_GEMM_TUNE APRIL_KW_FF1 APRIL_FULLK_NW8 APRIL_GEMM_LDSPAD APRIL_PP_SPLIT APRIL_PW_DEFER APRIL_PREFETCH
APRIL_CHAIN_STREAMS APRIL_STREAM_PRIO""".split()


def files_under(*dirs):
    for d in dirs:
        for base, _, names in os.walk(os.path.join(ROOT, d)):
            if "__pycache__" in base or os.sep + "build" in base:
                continue
            for n in names:
                if n.endswith((".cc", ".h", ".hip", ".inc", ".py", ".sh", ".c", ".cpp", ".md", ".txt", ".map")) or n == "Makefile":
                    yield os.path.join(base, n)


def test_environment_names_match_the_documented_table():
    literals = set()
    for path in files_under(os.path.join("april_asr_amd", "csrc")):
        with open(path, errors="replace") as f:
            literals.update(re.findall(r'"(APRIL_[A-Z0-9_]+)"', f.read()))
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    table = text[text.index("## Environment"):]
    rows = set(re.findall(r"^\| `(APRIL_[A-Z0-9_]+)` \|", table, flags=re.M))
    assert literals and literals == rows, (sorted(literals - rows), sorted(rows - literals))

    this = os.path.abspath(__file__)
    pat = re.compile(r"\b(%s)\b" % "|".join(REMOVED))
    hits = []
    for path in files_under("april_asr_amd", "tools", "tests", "examples"):
        if os.path.abspath(path) == this:
            continue
        with open(path, errors="replace") as f:
            for m in pat.finditer(f.read()):
                hits.append((os.path.relpath(path, ROOT), m.group(1)))
    assert not hits, hits
