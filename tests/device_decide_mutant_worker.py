"""Runs the reference-based checks of the plain search decision through the DEVICE's copy of it (csrc/kernels_misc.hip decide_kernel, via
aprilx_run_decide) of the library named by APRIL_ASR_LIB -- a mutant built by tests/mutate_device_decide.py.  Needs a GPU.
    python device_decide_mutant_worker.py MODEL.april [MODEL.april ...]
For every model: each hand-derived state-machine case (tests/golden/state_machine_cases.py) and the NaN row; for a model of 500 tokens or
more also the ties between ids of one lane.  The code is tests/test_gpu_decide.py's own.  Exit status 0 = every check passed (the
mutant SURVIVES), 1 = a check caught it."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import state_machine_cases as G  # noqa: E402


def main():
    import april_asr_amd as A
    from test_gpu_decide import check_hand_derived_case, check_nan_row, check_same_lane_ties
    from test_state_machine_golden import symbols
    for path in sys.argv[1:]:
        m = A.Model(path)
        tokens = [m.token(i) for i in range(m.dims.vocab)]
        sym = symbols(tokens)
        what = "%s: " % os.path.basename(path)
        try:
            for case in G.CASES:
                what = "%s %s: " % (os.path.basename(path), case["name"])
                check_hand_derived_case(m, case, sym)
            what = "%s NaN row: " % os.path.basename(path)
            check_nan_row(m, tokens)
            if m.dims.vocab >= 500:
                what = "%s same-lane ties: " % os.path.basename(path)
                check_same_lane_ties(m)
        except AssertionError as e:
            print("KILLED by %s%s" % (what, str(e)[:200].replace("\n", " ")))
            return 1
        m.close()
    print("SURVIVED")
    return 0


if __name__ == "__main__":
    sys.exit(main())
