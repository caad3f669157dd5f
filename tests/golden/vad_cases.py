"""Hand-derived cases of the voice-activity contract.  The band is ONE bin with inv_nb = 1, so a row's value is
its energy e; every energy is a small integer and every s, cur, d below a small integer or a multiple of 1/4: all sums are exact.
Thresholds thr_on = 2, thr_off = 1.  A case gives the energies, the bytes (st | raw << 1) worked out by hand in its comment, and
`mutant`: the one change of the reference (tests/vad_ref.py `mut`) under which the case must FAIL.

Where a case wants the smoothed value s to take given integer values, the energies follow from s' = s + (e - s) / 4, that is
e = s + 4 (s' - s): `energies_for`."""


def plan(onset=1, hang=1, min_energy=-100.0):
    return dict(b0=0, b1=1, inv_nb=1.0, thr_on=2.0, thr_off=1.0, min_energy=min_energy, onset_frames=onset, hangover_frames=hang)


def energies_for(s_values):
    e, s = [], None
    for x in s_values:
        e.append(x if s is None else s + 4 * (x - s))
        s = x
    return e


CASES = [
    # frame 0: s = 0, n = 0, d = 0.  frame 1: s = 0 + 8/4 = 2, n = 0, d = 2 == thr_on: not above, raw 0.  frame 2: s = 2 + 6/4 = 3.5,
    # d = 3.5: raw 1, run 1 < 2: byte 2
    dict(name="d_equals_thr_on", plan=plan(onset=2, hang=2), e=[0, 8, 8], want=[0, 0, 2], mutant="ge"),
    # s = 0, 4, 7: raw at frames 1, 2, run 2 = onset: st 1 at frame 2 (byte 3).  frame 3: e = -17: s = 7 - 24/4 = 1, n = 0,
    # d = 1 == thr_off: not above, raw 0, run 1 < 2: byte 1.  frame 4: e = 1: s = 1, d = 1: raw 0, run 2 = hangover: st 0, byte 0
    dict(name="d_equals_thr_off_and_hangover_reached", plan=plan(onset=2, hang=2), e=[0, 16, 16, -17, 1], want=[0, 2, 3, 1, 0], mutant="ge"),
    # onset 3: s = 0, 4, 7, 9.25: raw at frames 1, 2, 3; run reaches 3 at frame 3
    dict(name="onset_reached_exactly", plan=plan(onset=3, hang=2), e=[0, 16, 16, 16], want=[0, 2, 2, 3], mutant="onset_late"),
    # ... one short: frame 3: e = -13: s = 7 - 20/4 = 2, d = 2: raw 0, run back to 0; frame 4: e = 22: s = 7, raw 1, run 1
    dict(name="onset_one_short", plan=plan(onset=3, hang=2), e=[0, 16, 16, -13, 22], want=[0, 2, 2, 0, 2], mutant="ge"),
    # in speech from frame 2 (s = 7).  frame 3: s = 1, raw 0, run 1 (byte 1).  frame 4: e = 17: s = 1 + 16/4 = 5, d = 5: raw 1, run 0
    # (byte 3).  frame 5: e = -11: s = 5 - 16/4 = 1: raw 0, run 1 (byte 1).  frame 6: e = 1: raw 0, run 2 = hangover: st 0
    dict(name="hangover_one_short_then_reached", plan=plan(onset=2, hang=2), e=[0, 16, 16, -17, 17, -11, 1], want=[0, 2, 3, 1, 3, 1, 0], mutant="hang_late"),
    # s = 0 for frames 0..31: the 32nd frame (31) closes sub-window 0 with minimum 0.  s = 8 from frame 32: d = 8, raw 1, onset 1: st 1
    # (byte 3) while a sub-window still holds the 0.  Sub-window k covers frames 32 k .. 32 k + 31; the 9th (k = 8) closes at frame 287
    # and overwrites hist[0] -- AFTER that frame's d was taken (step 5 before step 7), so frame 287 is still 3.  Frame 288: every
    # minimum is 8, d = 0, raw 0, hangover 1: st 0, byte 0
    dict(name="ninth_sub_window_overwrites_the_first", plan=plan(), e=energies_for([0] * 32 + [8] * 257), want=[0] * 32 + [3] * 256 + [0], mutant="win9"),
    # the dip s = 0 sits ON the 32nd frame (31) of sub-window 0 (s = 4 before it: d = 0 throughout, and at frame 31 d = 0 - 0 = 0); s = 4
    # from frame 32: d = 4 until sub-window 0 is overwritten at frame 287.  Were a sub-window 33 frames, the dip would be forgotten later
    dict(name="thirty_second_frame_closes_the_sub_window", plan=plan(), e=energies_for([4] * 31 + [0] + [4] * 257), want=[0] * 32 + [3] * 256 + [0],
         mutant="sub33"),
    # min_energy -4: frame 0: e = -10 is raised to -4: s = -4.  frame 1: e = 4: s = -4 + 8/4 = -2, d = 2: not above thr_on.  Unclamped,
    # s = -10, then -6.5, d = 3.5: speech
    dict(name="energy_below_min_energy", plan=plan(min_energy=-4.0), e=[-10, 4], want=[0, 0], mutant="noclamp"),
    # the first frame after a reset takes s = e: s = 16, 16, d = 0.  Smoothed from 0 instead: s = 4, 7, d = 3 at frame 1: speech
    dict(name="first_frame_after_reset", plan=plan(), e=[16, 16], want=[0, 0], mutant="nofirst"),
    # a segment still open when the audio ends: s = 0, 4, 7, 7: st 1 from frame 2; a flush that completes here closes it
    dict(name="open_segment_at_flush", plan=plan(onset=2, hang=2), e=energies_for([0, 4, 7, 7]), want=[0, 2, 3, 3], mutant="onset_late"),
]

# events from bytes: frame shift 10 ms, the bytes are frames t0 .. of a session whose frame t0 - 1 was silence.
# onset 2, hangover 3.  0 -> 1 at frame 102: START at (102 - 2 + 1) * 10; 1 -> 0 at frame 106: END at (106 - 3 + 1) * 10
EVENT_CASES = [
    dict(onset=2, hang=3, shift=10, t0=100, data=[0, 2, 3, 3, 1, 1, 0, 0], want=[(1, 1010), (2, 1040)], last=0, open_end=[]),
    # still in speech at the end: the flush closes it at frames_seen * shift = (100 + 4) * 10
    dict(onset=2, hang=3, shift=10, t0=100, data=[0, 2, 3, 3], want=[(1, 1010)], last=1, open_end=[(2, 1040)]),
    # onset 1 at the session's first frame
    dict(onset=1, hang=1, shift=10, t0=0, data=[3, 0], want=[(1, 0), (2, 10)], last=0, open_end=[]),
]
