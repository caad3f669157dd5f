"""Hand-derived pins of the per-session search options.

DATA, not code under test: every expectation below was worked out by hand from the contract (the derivation is in the comments); nothing
here was produced by running the product or tests/search_options_ref.py.  Symbols as in state_machine_cases.py (W1, W2 word-start
tokens, C1, C2 continuation tokens, DOT "."), resolved by the tests against the model's token table; BLK is the blank.

A case: `opts` = None (no options) or (E, p, U); `rounds` = joiner rounds (token, max logit, blank logit, early_emit, now_ms) in order -- the
scripted joiner puts `max` on the token, `blank` on the blank id and -1000 everywhere else --; `events` = the callbacks, (kind, [(token,
logprob, flags, time_ms)...]) with flags 1 = WORD_BOUNDARY, 2 = SENTENCE_END; `expect` = per round what the device's decision leaves:
    (is_blank, (context[0], context[1]), last active token or None, time of the last emission, context changed)
`device` = False for the cases that only the host can tell apart (U).  Every session starts at context [BLK, BLK], nothing active,
last emission at 0, "silence already emitted" set.

Arithmetic used below (fp32): 6.5, 5.0, 1.5 and 2^-21 are exact; the spacing of fp32 in [4, 8) is 2^-21, so
nextafter(6.5, +inf) = 6.5 + 2^-21 and (6.5 + 2^-21) - 1.5 = 5 + 2^-21 exactly, the neighbour of 5.0."""
import numpy as np

P, F, S = "PARTIAL", "FINAL", "SILENCE"
BLK = "<blk>"
UP_6_5 = float(np.nextafter(np.float32(6.5), np.float32(np.inf)))


def _boundary(E, opts_given=True):
    """One word, then blank rounds at gaps E - 1, E and E + 40 behind it.
    r0 (W1, 5, 0, early 1, t 40): context[1] = BLK != W1 -> early stays 1; (0 - 0 - 1) > 5 false -> non-blank: last emission 40, context
       [BLK, W1], PARTIAL [W1 (5.0, WORD_BOUNDARY, 40)].
    r1 (C1, -20, 10, early 1, t 40 + E - 1): (10 - 1) > -20 -> blank; C1 is no punctuation.  gap = E - 1 < E: no endpoint.  decayed =
       -20 - gap / 3000 < 10 - 4: not confident; the refresh PARTIAL is suppressed (last call had 1 token, 1 is active).  Nothing.
    r2 (same, t 40 + E): gap = E >= E -> FINAL [W1]; the context starts with BLK, so the clear does nothing (quirk kept); SILENCE.
       Device: last token forgotten, context unchanged, not flagged as changed.
    r3 (same, t 40 + E + 40): gap > E again: nothing active, silence already emitted -> no call.  State unchanged."""
    w1 = ("W1", 5.0, 1, 40)
    return dict(
        name="endpoint_boundary_%d%s" % (E, "" if opts_given else "_no_options"), opts=(E, 0.0, 0) if opts_given else None, device=True,
        rounds=[("W1", 5.0, 0.0, 1.0, 40), ("C1", -20.0, 10.0, 1.0, 40 + E - 1), ("C1", -20.0, 10.0, 1.0, 40 + E), ("C1", -20.0, 10.0, 1.0, 40 + E + 40)],
        events=[(P, [w1]), (F, [w1]), (S, [])],
        expect=[(False, (BLK, "W1"), "W1", 40, True), (True, (BLK, "W1"), "W1", 40, False), (True, (BLK, "W1"), None, 40, False),
                (True, (BLK, "W1"), None, 40, False)])


CASES = [
    _boundary(200), _boundary(700), _boundary(2200), _boundary(60000),
    _boundary(2200, opts_given=False),              # the same script through a session without options: the literal 2200

    dict(
        name="endpoint_700_clears_a_two_token_context", opts=(700, 0.0, 0), device=True,
        # r0 W1 as above.  r1 (C1, 5, 0, early 0, t 40): (0 - 0) > 5 false -> non-blank: context [W1, C1], PARTIAL [W1, C1].
        # r2 (C2, -20, 10, early 1, t 739): gap 699 < 700: blank, not confident, nothing.
        # r3 (C2, -20, 10, early 1, t 740): gap 700 -> FINAL [W1, C1]; context[0] = W1 != BLK -> cleared to [BLK, BLK] (changed); SILENCE.
        # r4 (W2, 5, 0, early 1, t 780): a cleared context; (0 - 1) > 5 false -> non-blank: context [BLK, W2], PARTIAL [W2].
        rounds=[("W1", 5.0, 0.0, 1.0, 40), ("C1", 5.0, 0.0, 0.0, 40), ("C2", -20.0, 10.0, 1.0, 739), ("C2", -20.0, 10.0, 1.0, 740),
                ("W2", 5.0, 0.0, 1.0, 780)],
        events=[(P, [("W1", 5.0, 1, 40)]), (P, [("W1", 5.0, 1, 40), ("C1", 5.0, 0, 40)]), (F, [("W1", 5.0, 1, 40), ("C1", 5.0, 0, 40)]), (S, []),
                (P, [("W2", 5.0, 1, 780)])],
        expect=[(False, (BLK, "W1"), "W1", 40, True), (False, ("W1", "C1"), "C1", 40, True), (True, ("W1", "C1"), "C1", 40, False),
                (True, (BLK, BLK), None, 40, True), (False, (BLK, "W2"), "W2", 780, True)]),

    dict(
        name="penalty_blank_test_at_5_exactly", opts=(2200, 1.5, 0), device=True,
        # r1 (C1, 5, 6.5, early 0, t 40): bl' = 6.5 - 1.5 = 5.0; (5.0 - 0) > 5.0 false -> NON-blank (raw: 6.5 > 5 would be blank):
        # context [W1, C1], PARTIAL [W1, C1 (5.0)].
        rounds=[("W1", 5.0, 0.0, 1.0, 40), ("C1", 5.0, 6.5, 0.0, 40)],
        events=[(P, [("W1", 5.0, 1, 40)]), (P, [("W1", 5.0, 1, 40), ("C1", 5.0, 0, 40)])],
        expect=[(False, (BLK, "W1"), "W1", 40, True), (False, ("W1", "C1"), "C1", 40, True)]),
    dict(
        name="penalty_blank_test_one_ulp_above", opts=(2200, 1.5, 0), device=True,
        # r1 (C1, 5, 6.5 + 2^-21, early 0, t 40): bl' = 5 + 2^-21 > 5.0 -> blank.  gap 0; decayed = 5.0 > bl' - 4 = 1 + 2^-21 and C1 != W1 ->
        # confident: provisional C1 with logprob 5 - 8 = -3, PARTIAL [W1, C1'], then the head goes back to 1.  Device state unchanged.
        rounds=[("W1", 5.0, 0.0, 1.0, 40), ("C1", 5.0, UP_6_5, 0.0, 40)],
        events=[(P, [("W1", 5.0, 1, 40)]), (P, [("W1", 5.0, 1, 40), ("C1", -3.0, 0, 40)])],
        expect=[(False, (BLK, "W1"), "W1", 40, True), (True, (BLK, "W1"), "W1", 40, False)]),

    dict(
        name="penalty_in_the_punctuation_override", opts=(2200, 5.0, 0), device=True,
        # r1 (DOT, 2, 10, early 0, t 40): bl' = 5; (5 - 0) > 2 -> blank by the logits (with and without p).  "." after the word W1 is a sentence
        # end; the context is not cleared (context[1] = W1), DOT != W1; 2 > 5 - 3.5 = 1.5 -> the override makes it NON-blank (raw: 2 > 6.5 false).
        # Emitted with SENTENCE_END: PARTIAL [W1, . (2.0, 2)]; context [W1, DOT].
        rounds=[("W1", 5.0, 0.0, 1.0, 40), ("DOT", 2.0, 10.0, 0.0, 40)],
        events=[(P, [("W1", 5.0, 1, 40)]), (P, [("W1", 5.0, 1, 40), ("DOT", 2.0, 2, 40)])],
        expect=[(False, (BLK, "W1"), "W1", 40, True), (False, ("W1", "DOT"), "DOT", 40, True)]),
    dict(
        name="no_penalty_no_override", opts=(2200, 0.0, 0), device=True,
        # the same script with p = 0: 10 > 2 blank; 2 > 10 - 3.5 false: stays blank.  decayed = 2 > 10 - 4 false: not confident; nothing.
        rounds=[("W1", 5.0, 0.0, 1.0, 40), ("DOT", 2.0, 10.0, 0.0, 40)],
        events=[(P, [("W1", 5.0, 1, 40)])],
        expect=[(False, (BLK, "W1"), "W1", 40, True), (True, (BLK, "W1"), "W1", 40, False)]),

    dict(
        name="penalty_in_the_provisional_token_test", opts=(2200, 5.0, 0), device=True,
        # r1 (C1, 2, 10, early 0, t 40): bl' = 5; 5 > 2 -> blank (raw 10 > 2 as well); C1 is no punctuation: no override.  gap 0: decayed =
        # 2.0 > bl' - 4 = 1.0 -> confident (raw: 2 > 6 false): provisional C1, logprob 2 - 8 = -6: PARTIAL [W1, C1'].
        rounds=[("W1", 5.0, 0.0, 1.0, 40), ("C1", 2.0, 10.0, 0.0, 40)],
        events=[(P, [("W1", 5.0, 1, 40)]), (P, [("W1", 5.0, 1, 40), ("C1", -6.0, 0, 40)])],
        expect=[(False, (BLK, "W1"), "W1", 40, True), (True, (BLK, "W1"), "W1", 40, False)]),
    dict(
        name="no_penalty_no_provisional_token", opts=(2200, 0.0, 0), device=True,
        # p = 0: blank, 2 > 10 - 4 false: nothing
        rounds=[("W1", 5.0, 0.0, 1.0, 40), ("C1", 2.0, 10.0, 0.0, 40)],
        events=[(P, [("W1", 5.0, 1, 40)])],
        expect=[(False, (BLK, "W1"), "W1", 40, True), (True, (BLK, "W1"), "W1", 40, False)]),

    dict(
        name="negative_penalty_favours_the_blank", opts=(2200, -1.5, 0), device=True,
        # r1 (C1, 5, 3.75, early 0, t 40): bl' = 3.75 + 1.5 = 5.25 > 5 -> blank (raw: 3.75 > 5 false).  decayed 5 > 5.25 - 4 -> provisional C1 (-3).
        rounds=[("W1", 5.0, 0.0, 1.0, 40), ("C1", 5.0, 3.75, 0.0, 40)],
        events=[(P, [("W1", 5.0, 1, 40)]), (P, [("W1", 5.0, 1, 40), ("C1", -3.0, 0, 40)])],
        expect=[(False, (BLK, "W1"), "W1", 40, True), (True, (BLK, "W1"), "W1", 40, False)]),
    dict(
        name="negative_penalty_at_5_exactly", opts=(2200, -1.5, 0), device=True,
        # r1 (C1, 5, 3.5, early 0, t 40): bl' = 5.0; 5.0 > 5.0 false -> non-blank
        rounds=[("W1", 5.0, 0.0, 1.0, 40), ("C1", 5.0, 3.5, 0.0, 40)],
        events=[(P, [("W1", 5.0, 1, 40)]), (P, [("W1", 5.0, 1, 40), ("C1", 5.0, 0, 40)])],
        expect=[(False, (BLK, "W1"), "W1", 40, True), (False, ("W1", "C1"), "C1", 40, True)]),

    # ---- the utterance cap U (host only).  All rounds (tok, 5, 0): (0 - early) > 5 false -> non-blank.
    dict(
        name="cap_one_ms_short", opts=(2200, 0.0, 1000), device=False,
        # W1 at t 40 is the utterance's first token (first = 40).  W2 at t 1039: a word boundary with 2 tokens active, 1039 - 40 = 999 < 1000:
        # no FINAL, PARTIAL with all three.
        rounds=[("W1", 5.0, 0.0, 1.0, 40), ("C1", 5.0, 0.0, 0.0, 40), ("W2", 5.0, 0.0, 1.0, 1039)],
        events=[(P, [("W1", 5.0, 1, 40)]), (P, [("W1", 5.0, 1, 40), ("C1", 5.0, 0, 40)]),
                (P, [("W1", 5.0, 1, 40), ("C1", 5.0, 0, 40), ("W2", 5.0, 1, 1039)])],
        expect=[(False, (BLK, "W1"), "W1", 40, True), (False, ("W1", "C1"), "C1", 40, True), (False, ("C1", "W2"), "W2", 1039, True)]),
    dict(
        name="cap_reached", opts=(2200, 0.0, 1000), device=False,
        # W2 at t 1040: 1040 - 40 = 1000 >= 1000 -> FINAL [W1, C1] before the word, then PARTIAL [W2] alone; no SILENCE, the context is kept
        # ([C1, W2]).  W2 becomes the next utterance's first token (first = 1040): W1 at t 2039 (999 later) finalises nothing.
        rounds=[("W1", 5.0, 0.0, 1.0, 40), ("C1", 5.0, 0.0, 0.0, 40), ("W2", 5.0, 0.0, 1.0, 1040), ("W1", 5.0, 0.0, 1.0, 2039)],
        events=[(P, [("W1", 5.0, 1, 40)]), (P, [("W1", 5.0, 1, 40), ("C1", 5.0, 0, 40)]), (F, [("W1", 5.0, 1, 40), ("C1", 5.0, 0, 40)]),
                (P, [("W2", 5.0, 1, 1040)]), (P, [("W2", 5.0, 1, 1040), ("W1", 5.0, 1, 2039)])],
        expect=[(False, (BLK, "W1"), "W1", 40, True), (False, ("W1", "C1"), "C1", 40, True), (False, ("C1", "W2"), "W2", 1040, True),
                (False, ("W2", "W1"), "W1", 2039, True)]),
    dict(
        name="cap_needs_a_word_boundary", opts=(2200, 0.0, 1000), device=False,
        # C2 at t 3040, far past U, continues a word: no FINAL
        rounds=[("W1", 5.0, 0.0, 1.0, 40), ("C1", 5.0, 0.0, 0.0, 40), ("C2", 5.0, 0.0, 1.0, 3040)],
        events=[(P, [("W1", 5.0, 1, 40)]), (P, [("W1", 5.0, 1, 40), ("C1", 5.0, 0, 40)]),
                (P, [("W1", 5.0, 1, 40), ("C1", 5.0, 0, 40), ("C2", 5.0, 0, 3040)])],
        expect=[(False, (BLK, "W1"), "W1", 40, True), (False, ("W1", "C1"), "C1", 40, True), (False, ("C1", "C2"), "C2", 3040, True)]),
    dict(
        name="cap_with_nothing_active", opts=(2200, 0.0, 1000), device=False,
        # the first token of all arrives at t 5000 (>= U after the stale first = 0) with nothing active: no FINAL; it sets first = 5000, so W2
        # at t 5999 (999 later) finalises nothing either
        rounds=[("W1", 5.0, 0.0, 1.0, 5000), ("W2", 5.0, 0.0, 1.0, 5999)],
        events=[(P, [("W1", 5.0, 1, 5000)]), (P, [("W1", 5.0, 1, 5000), ("W2", 5.0, 1, 5999)])],
        expect=[(False, (BLK, "W1"), "W1", 5000, True), (False, ("W1", "W2"), "W2", 5999, True)]),
]

# (E, p, U, size delta) that aprilx_session_set_search_options refuses; the previous options stay in place
REFUSED = [(199, 0.0, 0, 0), (60001, 0.0, 0, 0), (700, float("nan"), 0, 0), (700, float("inf"), 0, 0), (700, float("-inf"), 0, 0), (700, 100.5, 0, 0),
           (700, 0.0, 999, 0), (700, 0.0, 600001, 0), (700, 0.0, 0, 4), (700, 0.0, 0, -4)]
ACCEPTED = [(200, 0.0, 0), (60000, 100.0, 600000), (700, -100.0, 1000), (2200, 0.0, 0)]
