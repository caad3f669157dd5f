"""The mutation yardsticks of the device decision (tests/mutate_device_decide.py) edit source text: a refactor of csrc/kernels_misc.hip,
kernels_bias.inc or kernels_confidence.inc that changes a line a mutant names would turn that mutant into a build failure which shows
only on a machine with a GPU.  This test needs none."""
import os

import mutate_device_decide as DM


def test_every_mutant_names_text_that_occurs_once():
    src = DM.read_sources()
    entries = DM.all_entries()
    assert len(DM.MUTANTS) >= 30 and len(DM.OPTIN_MUTANTS) >= 36 and len(entries) == len(DM.MUTANTS) + len(DM.EQUIVALENT) + len(DM.OPTIN_MUTANTS) + len(DM.OPTIN_EQUIVALENT)
    for names in ([m[0] for m in DM.MUTANTS], [m[0] for m in DM.EQUIVALENT], [m[0] for m in DM.OPTIN_MUTANTS], [m[0] for m in DM.OPTIN_EQUIVALENT]):
        assert len(set(names)) == len(names), "two mutants of one list share a name (they would share a directory)"
    for name, fname, old, new in entries:
        assert fname in DM.FILES and os.path.exists(os.path.join(DM.CSRC, fname)), (name, fname)
        assert src[fname].count(old) == 1, "%s: its original text occurs %d times in %s" % (name, src[fname].count(old), fname)
        assert new != old, "%s: the replacement is the original" % name
    for m in DM.OPTIN_EQUIVALENT:
        assert len(m) == 5 and len(m[4]) > 20, "%s: an equivalent mutant needs its argument" % m[0]
