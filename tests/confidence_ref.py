"""The contract of the per-token confidences in float64, and its error bound: shared by
tests/test_confidence_cpu.py (which checks this file on its own) and tests/test_gpu_confidence.py (which checks the device against it).

For one joiner evaluation with fp32 logits v[0..V), blank included:
    M = max v,  S = sum exp(v - M),  lse = M + log S,  log_softmax(n) = v[n] - lse
    alternatives: the non-blank ids ordered by v descending, lower id first on equal values, the first K
    no non-blank logit above the search's initial value -9999999999 (a NaN row): n_alt = 0, lse = NaN
"""
import numpy as np

INITIAL = np.float32(-9999999999.0)          # the arg-max's initial value (reference src/april_session.c:311)


def reference(row, blank, k):
    """(lse64, alt ids, alt logits as fp32, blank log-softmax in float64) of one fp32 logits row"""
    row = np.asarray(row, np.float32)
    v = row.astype(np.float64)
    ids = np.array([n for n in range(row.size) if n != blank and not np.isnan(row[n])], np.int64)
    if ids.size == 0 or not (row[ids] > INITIAL).any():
        return float("nan"), np.zeros(0, np.int64), np.zeros(0, np.float32), float("nan")
    order = ids[np.lexsort((ids, -v[ids]))][:k]            # value descending, then id ascending
    m = v.max()
    lse = m + np.log(np.exp(v - m).sum())
    return float(lse), order, row[order], float(v[blank] - lse)


def lse_bound(lse64):
    """|lse - lse64| allowed: exp and log within 1 ulp + the argument rounding, <= 32 additions per term, two final roundings"""
    return 3e-6 + 2.0 ** -23 * abs(lse64)


def ls_bound(lse64, ls64):
    return 3e-6 + 2.0 ** -23 * (abs(lse64) + abs(ls64))


def lse_fp32_emulation(rows):
    """One legal fp32 evaluation order of lse for rows [R][V]: 256 lane-strided partial sums (lane t adds n = t, t + 256, ... in
    order), an xor butterfly inside each group of 64 lanes, then the four group sums ((w0 + w1) + w2) + w3; numpy's float32 exp / log."""
    rows = np.asarray(rows, np.float32)
    r, v = rows.shape
    m = rows.max(axis=1, keepdims=True)
    e = np.exp((rows - m).astype(np.float32)).astype(np.float32)
    j = (v + 255) // 256
    pad = np.zeros((r, j * 256), np.float32)
    pad[:, :v] = e                                           # (a missing term adds +0.0 to a positive sum: no change)
    pad = pad.reshape(r, j, 256)
    lane = np.zeros((r, 256), np.float32)
    for q in range(j):
        lane = (lane + pad[:, q, :]).astype(np.float32)
    w = lane.reshape(r, 4, 64)
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = (w + w[:, :, idx ^ off]).astype(np.float32)
    w = w[:, :, 0]
    s = (((w[:, 0] + w[:, 1]).astype(np.float32) + w[:, 2]).astype(np.float32) + w[:, 3]).astype(np.float32)
    return (m[:, 0] + np.log(s).astype(np.float32)).astype(np.float32)


def random_rows(rng, n, vocab, scale, offset=300.0):
    return (rng.standard_normal((n, vocab)) * scale + rng.uniform(-offset, offset, size=(n, 1))).astype(np.float32)


def check_info(info, row, blank, k, what=""):
    """One AprilxTokenInfo (ctypes) against the float64 reference on `row`: ids exact, logits bitwise, lse and every log-softmax
    inside the bound.  Returns the largest error / bound ratio seen."""
    lse64, ids, logits, blank_ls64 = reference(row, blank, k)
    assert int(info.n_alt) == ids.size, "%s: n_alt %d, reference %d" % (what, info.n_alt, ids.size)
    if ids.size == 0:
        assert np.isnan(info.lse), what
        return 0.0
    got_ids = [int(info.alt_id[i]) for i in range(ids.size)]
    assert got_ids == [int(x) for x in ids], "%s: alternatives %r, reference %r" % (what, got_ids, list(ids))
    got_lg = np.array([info.alt_logit[i] for i in range(ids.size)], np.float32)
    assert np.array_equal(got_lg.view(np.uint32), logits.view(np.uint32)), "%s: alternative logits are not the input bits" % what
    worst = abs(float(info.lse) - lse64) / lse_bound(lse64)
    assert worst <= 1.0, "%s: lse %r vs %r: %.3g of the bound" % (what, float(info.lse), lse64, worst)
    cases = [(float(info.token_logprob), float(logits[0]) - lse64), (float(info.blank_logprob), blank_ls64)]
    cases += [(float(np.float32(info.alt_logit[i]) - np.float32(info.lse)), float(logits[i]) - lse64) for i in range(ids.size)]
    for got, want in cases:
        ratio = abs(got - want) / ls_bound(lse64, want)
        assert ratio <= 1.0, "%s: log-softmax %r vs %r: %.3g of the bound" % (what, got, want, ratio)
        worst = max(worst, ratio)
    return worst
