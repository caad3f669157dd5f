"""Ramp merge, the part that needs no GPU (csrc/engine.cc ramp_window through aprilx_ramp_window): which
problems of the next feed's first R macro steps the last R macro steps of a feed hold.  At macro step W (1-based) of a feed of T
chunks over L layers, layer l works on chunk W - 1 - l; the feed's last chunk T - 1 therefore passes layer l at step T + l."""
import numpy as np
import pytest

from april_asr_amd import _ffi

R = 2


def window(L, T, r=R):
    out = np.full(64, -7, np.int32)
    n = _ffi.lib().aprilx_ramp_window(L, T, r, out.ctypes.data, out.size)
    assert n >= 0
    stride = 3 + 2 * r
    steps = []
    for i in range(n):
        rec = out[i * stride:(i + 1) * stride]
        guests = [(int(rec[3 + 2 * g]), int(rec[4 + 2 * g])) for g in range(int(rec[2]))]
        assert all(int(x) == -1 for x in rec[3 + 2 * int(rec[2]):])
        steps.append((int(rec[0]), int(rec[1]), guests))
    return steps


def own_problems(L, T, W):
    return [(l, W - 1 - l) for l in range(L) if 0 <= W - 1 - l < T]


@pytest.mark.parametrize("L", [12, 16])
@pytest.mark.parametrize("T", range(1, 8))
def test_window_of_a_feed(built, L, T):
    steps = window(L, T)
    assert len(steps) == R, "every feed of these shapes is hosted"
    assert [s[0] for s in steps] == [L + T - 1 - R + j for j in range(1, R + 1)]
    # every head problem of the next feed's steps 1..R appears as a guest exactly once (the guest feed's own chunk count masks
    # the chunks it does not have on the device: the plan holds them all)
    head = [(l, W - 1 - l) for W in range(1, R + 1) for l in range(L) if 0 <= W - 1 - l < R]
    guests = [g for _, _, gs in steps for g in gs]
    assert sorted(guests) == sorted(head) and len(set(guests)) == len(guests)
    for j, (W, own, gs) in enumerate(steps, start=1):
        assert own == len(own_problems(L, T, W))
        assert own + len(gs) <= 3
        # guests of window step j are the problems of the next feed's macro step j
        assert sorted(gs) == sorted((l, t) for (l, t) in head if l + t + 1 == j)
        for (l, t) in gs:
            assert W > T + l, "the host feed's last chunk passed layer %d at step %d" % (l, T + l)
            assert W <= L + T - 1, "inside the host's own macro steps"
    # chunk t + 1 of a layer after chunk t, layer l + 1 of a chunk after layer l: in different window steps, in order
    at = {g: W for W, _, gs in steps for g in gs}
    for (l, t), W in at.items():
        assert all(at[(l, t - 1)] < W for _ in [0] if (l, t - 1) in at) and all(at[(l - 1, t)] < W for _ in [0] if (l - 1, t) in at)
    if T == 1:
        assert max(len(gs) for _, _, gs in steps) <= 2 and [s[1] for s in steps] == [1, 1]
    if T >= 4:
        assert [s[1] for s in steps] == [2, 1]


def test_window_refuses_what_it_cannot_hold(built):
    assert window(4, 2) == [] and window(3, 3) == []         # the window would reach into the feed's own head (L <= 2 R)
    assert window(5, 2) != []
    assert window(12, 3, r=3) == []                          # R = 3 would ask for four problems per launch
    out = np.zeros(4, np.int32)
    assert _ffi.lib().aprilx_ramp_window(12, 2, 2, out.ctypes.data, out.size) == -1      # no room
    assert _ffi.lib().aprilx_ramp_window(0, 2, 2, out.ctypes.data, out.size) == -1
    assert _ffi.lib().aprilx_ramp_window(12, 2, 2, None, 64) == -1
