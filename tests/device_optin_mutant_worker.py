"""Runs the reference-based checks of the search decision's OPT-IN lines -- phrase boosting and strict sets (csrc/kernels_bias.inc), search
options (the OPT lines of decide_body), confidences (csrc/kernels_confidence.inc) -- through the library named by APRIL_ASR_LIB: a mutant
built by tests/mutate_device_decide.py.  Needs a GPU.
    python device_optin_mutant_worker.py BLANK39.april BLANK1050.april
For every model, through aprilx_run_decide_biased, aprilx_run_decide_opts, aprilx_run_confidence and aprilx_run_confidence_biased: the rows of
tests/test_gpu_confidence.py against confidence_ref (K = 1, 4, 8), the scripted and random rounds of tests/test_gpu_bias.py against bias_ref,
the given rows and the confidences over the permitted subset of tests/test_gpu_bias_strict.py against bias_strict_ref, the mixed rows, the
hand-derived cases and the return to the root of tests/test_gpu_search_options.py against search_options_ref.  The code is those
files' own.  Exit status 0 = every check passed (the mutant SURVIVES), 1 = a check caught it."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))


def main():
    import april_asr_amd as A
    import search_options_worker as W
    import test_gpu_bias as TB
    import test_gpu_bias_strict as TS
    import test_gpu_confidence as TC
    import test_gpu_search_options as TO
    for path in sys.argv[1:]:
        gm, host = A.Model(path), A.Model.load_host_only(path)
        sym = W.symbols([gm.token(i) for i in range(gm.dims.vocab)])
        checks = [("confidences against float64", lambda: TC.check_kernel_against_float64(gm, os.path.basename(path))),
                  ("boosting sets, scripted and random rounds", lambda: TB.check_scripted_rounds(gm)),
                  ("strict sets, given rows", lambda: TS.check_given_rows(gm)),
                  ("strict sets, confidences over the permitted subset", lambda: TS.check_confidences_over_the_permitted_subset(gm)),
                  ("search options, mixed rows", lambda: TO.check_mixed_rows(gm)),
                  ("search options, back to the root at E", lambda: [TO.check_bias_state_returns_to_the_root_at_E(gm, s) for s in (False, True)])]
        checks += [("search options, " + c["name"], (lambda c=c: TO.check_device_case(gm, host, c, sym))) for c in TO.DEVICE_CASES]
        for what, fn in checks:
            try:
                fn()
            except AssertionError as e:
                print("KILLED by %s on %s: %s" % (what, os.path.basename(path), str(e)[:200].replace("\n", " ")))
                return 1
        host.close(); gm.close()
    print("SURVIVED")
    return 0


if __name__ == "__main__":
    sys.exit(main())
