"""Mutation test of the search-option fixtures (tests/golden/search_options_cases.py) against the lines DESIGN.md section 14 adds to the
product's host state machine (csrc/session.cc `Greedy`), in the style of tests/mutate_product_state_machine.py: single edits of those
lines, each compiled (g++ on the one host source, linked with the library's other objects into its own .so) and run through
aprilx_greedy_* of that library (tests/search_options_worker.py, host-only, APRIL_ASR_LIB).  A mutant that passes every case SURVIVES; the
run fails unless there are none.

usage: python tests/mutate_search_options.py [-v]      (tests/test_search_options_cpu.py runs it inside the CPU suite)
"""
import glob
import os
import shutil
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mutate_product_state_machine as MP  # noqa: E402

ROOT, CSRC = MP.ROOT, MP.CSRC
W = "APRIL_TOKEN_FLAG_WORD_BOUNDARY_BIT"
ENDPOINT = "if (has_opt_) endpoint = gap >= (size_t)endpoint_ms_;"
PENALTY = "has_opt_ ? blank_raw - blank_penalty_ : blank_raw;"
CAP = "if (has_opt_ && max_utt_ms_ && head_ > 0 && (flags & %s) && now_ms - first_ms_ >= (size_t)max_utt_ms_) fin = true;" % W
# (name, text in csrc/session.cc -- must occur exactly once --, replacement)
MUTANTS = [
    ("endpoint_strictly_after_E", ENDPOINT, ENDPOINT.replace("gap >=", "gap >")),
    ("endpoint_after_E_plus_1", ENDPOINT, ENDPOINT.replace("(size_t)endpoint_ms_", "(size_t)endpoint_ms_ + 1")),
    ("endpoint_after_E_minus_1", ENDPOINT, ENDPOINT.replace("(size_t)endpoint_ms_", "(size_t)endpoint_ms_ - 1")),
    ("penalty_added", PENALTY, PENALTY.replace("blank_raw - blank_penalty_", "blank_raw + blank_penalty_")),
    ("no_penalty_in_the_blank_test", "bool is_blank = (blank_v - early_emit) > best_v;", "bool is_blank = (blank_raw - early_emit) > best_v;"),
    ("no_penalty_in_the_override", "best_v > (blank_v - 3.5f)) is_blank = false;", "best_v > (blank_raw - 3.5f)) is_blank = false;"),
    ("no_penalty_in_the_provisional_test", "decayed > (blank_v - 4.0f);", "decayed > (blank_raw - 4.0f);"),
    ("cap_strictly_after_U", CAP, CAP.replace("first_ms_ >=", "first_ms_ >")),
    ("cap_without_word_boundary", CAP, CAP.replace(" && (flags & %s)" % W, "")),
]


def run_mutant(tmp, objs, src, name, old, new, model_path):
    """MP.run_mutant with this file's worker"""
    import subprocess
    if src.count(old) != 1:
        return "FAILED", "the text to mutate occurs %d times in session.cc" % src.count(old)
    so, why = MP.build_variant(tmp, name, src.replace(old, new), objs)
    if so is None:
        return "FAILED", why
    env = dict(os.environ, APRIL_ASR_LIB=so, APRIL_LOG_LEVEL="NONE")
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "search_options_worker.py"), model_path], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    except subprocess.TimeoutExpired:
        return "KILLED", "time-out"
    finally:
        for f in (so, os.path.join(tmp, name + ".o"), os.path.join(tmp, name + ".cc")):
            try:
                os.remove(f)
            except OSError:
                pass
    out = r.stdout.decode()
    if r.returncode == 0 and "SURVIVED" in out:
        return "SURVIVED", ""
    return "KILLED", (out.strip().splitlines() or ["exit %d" % r.returncode])[-1][:200]


def run_all(verbose=False, model_path=None, workers=6):
    """returns (killed, survivors, build_failures)"""
    src = open(os.path.join(CSRC, "session.cc")).read()
    objs = [o for o in sorted(glob.glob(os.path.join(CSRC, "build", "*.o"))) if os.path.basename(o) != "session.o"]
    assert objs, "build the library first (csrc/build/*.o)"
    tmp = tempfile.mkdtemp(prefix="april_somutants_")
    try:
        if model_path is None:
            sys.path.insert(0, ROOT)
            from april_asr_amd import synth_model as SM
            model_path = os.path.join(tmp, "tiny.april")
            SM.write_model(model_path, SM.TINY_DIMS)
        status, why = run_mutant(tmp, objs, src, "identity", "bool Greedy::on_joint(", "bool Greedy::on_joint(", model_path)
        assert status == "SURVIVED", "the unmutated product fails the fixtures through this harness: %s" % why
        with ThreadPoolExecutor(workers) as ex:
            res = list(ex.map(lambda m: (m[0],) + run_mutant(tmp, objs, src, m[0], m[1], m[2], model_path), MUTANTS))
        killed, survivors, failures = [], [], []
        for name, status, why in res:
            if verbose:
                print("%-42s %s %s" % (name, status, why))
            (killed if status == "KILLED" else survivors if status == "SURVIVED" else failures).append((name, why))
        return killed, survivors, failures
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    k, s, f = run_all(verbose="-v" in sys.argv)
    print("%d mutants of the search-option lines of csrc/session.cc: %d killed, %d survived, %d failed to build" % (len(MUTANTS), len(k), len(s), len(f)))
    for name, _ in s:
        print("SURVIVOR:", name)
    for name, why in f:
        print("BUILD FAILURE:", name, why)
    sys.exit(1 if (s or f) else 0)
