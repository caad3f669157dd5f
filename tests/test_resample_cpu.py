"""Input sample rates (aprilx_resampler_taps, no GPU): the phase table the library exports is the contract's formula (DESIGN.md
section 11) evaluated in float64 and rounded once, the rate limits hold, and the filter's response meets its figures."""
import numpy as np
import pytest

import april_asr_amd as A

TO_16K = [8000, 11025, 22050, 32000, 44100, 48000, 96000]
# the edges of the accepted space: upsampling with a small L (4000, 12000 Hz), L = 4000 (4004, 16204, 383996 Hz: the largest phase
# tables), K = 854 (384000 Hz), model rates other than 16 kHz, and 328000 Hz at an 8 kHz model (the largest LDS span accepted)
EDGE_PAIRS = [(4000, 16000), (4004, 16000), (12000, 16000), (16204, 16000), (383996, 16000), (384000, 16000),
              (8000, 44100), (16000, 44100), (384000, 44100), (16000, 8000), (48000, 8000), (328000, 8000)]
PAIRS = [(r, 16000) for r in TO_16K] + [(48000, 44100)] + EDGE_PAIRS


def contract_lmk(ri, ro):
    g = np.gcd(ri, ro)
    lo = min(ri, ro)
    return ro // g, ri // g, -((-320 * ri) // (9 * lo))


def contract_taps(ri, ro):
    """tap[p][i] = (2 fc / R_i) sinc(2 fc tau) w(tau / T), tau = (p / L + K - 1 - i) / R_i, in float64"""
    L, M, K = contract_lmk(ri, ro)
    fc = 0.45 * min(ri, ro)
    T = 32.0 / (2.0 * fc)
    p = np.arange(L, dtype=np.float64)[:, None]
    i = np.arange(2 * K, dtype=np.float64)[None, :]
    tau = (p / L + K - 1 - i) / ri
    u = tau / T
    w = np.where(np.abs(u) < 1, np.i0(8.6 * np.sqrt(np.clip(1 - u * u, 0, None))) / np.i0(8.6), 0.0)
    return (2 * fc / ri) * np.sinc(2 * fc * tau) * w, tau


@pytest.mark.parametrize("ri,ro", PAIRS)
def test_taps_match_the_contract(built, ri, ro):
    L, M, K, taps = A.resampler_taps(ri, ro)
    assert (L, M, K) == contract_lmk(ri, ro)
    ref, _ = contract_taps(ri, ro)
    assert taps.shape == (L, 2 * K)
    tol = np.maximum(np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64), 1e-9)
    err = np.abs(taps.astype(np.float64) - ref)
    assert (err <= tol).all(), "worst tap off by %g (tolerance there %g)" % (err.max(), tol.ravel()[err.argmax()])
    sums = taps.astype(np.float64).sum(axis=1)
    assert np.abs(sums - 1).max() <= 1e-4, np.abs(sums - 1).max()


def test_worked_numbers(built):
    assert A.resampler_taps(48000, 16000)[:3] == (1, 3, 107)
    assert A.resampler_taps(44100, 16000)[:3] == (160, 441, 98)
    assert A.resampler_taps(8000, 16000)[:3] == (2, 1, 36)
    assert A.resampler_taps(16000, 16000)[:3] == (1, 1, 0)        # no conversion


@pytest.mark.parametrize("ri,ro", [(0, 16000), (3999, 16000), (384001, 16000), (4001, 16000), (383999, 16000),
                                   (336000, 8000), (383996, 44100)])
def test_refused(built, ri, ro):
    from april_asr_amd import _ffi
    lmk = np.zeros(3, np.int32)
    assert _ffi.lib().aprilx_resampler_taps(ri, ro, lmk.ctypes.data, None, 0) == -1
    with pytest.raises(ValueError):
        A.resampler_taps(ri, ro)


def test_limits_accepted(built):
    # the ends of the range are accepted when L stays <= 4096 (4000 -> 16000: L 4; 384000 -> 16000: M 24)
    assert A.resampler_taps(4000, 16000)[:2] == (4, 1)
    assert A.resampler_taps(384000, 16000)[:2] == (1, 24)
    assert contract_lmk(4001, 16000)[0] > 4096


@pytest.mark.parametrize("ri,ro", PAIRS)
def test_response(built, ri, ro):
    """The exported table applied in float64: every phase is flat to 0.01 dB up to 0.8 of the lower Nyquist frequency, and the
    prototype filter (all phases interleaved, at L x R_i) is down by 85 dB or more from the lower Nyquist frequency on."""
    L, M, K, taps = A.resampler_taps(ri, ro)
    t = taps.astype(np.float64)
    _, tau = contract_taps(ri, ro)
    ny = min(ri, ro) / 2.0
    fp = np.linspace(0.0, 0.8 * ny, 256)
    for p in range(0, L, max(1, L // 8)):
        g = np.abs(np.exp(-2j * np.pi * fp[:, None] * tau[p][None, :]) @ t[p])
        assert np.abs(20 * np.log10(g)).max() <= 0.01, (p, np.abs(20 * np.log10(g)).max())
    if t.size <= 100000:
        fs = np.linspace(ny, L * ri / 2.0, 2048)
        tr, taur = t.ravel(), tau.ravel()
        h = np.zeros(fs.size, np.complex128)
        for c in range(0, tr.size, 16384):          # (in pieces of taps: the same sum, a bounded matrix)
            h += np.exp(-2j * np.pi * fs[:, None] * taur[None, c:c + 16384]) @ tr[c:c + 16384]
        h = np.abs(h) / L
    else:
        # L = 4000: the prototype's taps sit on the grid m / (L R_i), m = p + L (K - 1 - i); its response on a zero-padded FFT
        # grid (spacing below 100 Hz), every bin from the lower Nyquist frequency to L R_i / 2
        proto = np.zeros(2 * L * K)
        m = np.arange(L)[:, None] + L * (K - 1 - np.arange(2 * K))[None, :] + L * K
        proto[m.ravel()] = t.ravel()
        nfft = 1 << int(np.ceil(np.log2(max(proto.size, L * ri / 100.0))))
        spec = np.abs(np.fft.rfft(proto, nfft)) / L
        f = np.arange(spec.size) * (L * ri / float(nfft))
        h = spec[f >= ny]
    assert 20 * np.log10(h.max()) <= -85.0, 20 * np.log10(h.max())
