"""The CPU model of the input sample-rate conversion (oracle/orc_resample.c; no GPU): the exact reference of the bit-exact kernel test
(tests/test_gpu_resample.py::test_kernel_bit_exact_against_the_contract).  Its fp32 FMA chain stays within the a-priori error bound
of a float64 evaluation at every pair of the kernel test's matrix; on the very inputs that test feeds, each deliberately different
summation (reversed taps, unfused multiply-add, two partial sums, a float64 accumulator) changes int16 outputs at every pair, so a
kernel that summed that way would fail it; and the plan's edges (L = 4000, the LDS budget, L > 4096) hold."""
from fractions import Fraction

import numpy as np
import pytest

import april_asr_amd as A
from oracle import orc_py as O
from resample_worker import EXACT_MATRIX, exact_cases

MATRIX = [(ri, ro) for ro, rates in EXACT_MATRIX.items() for ri in rates]
U = 2.0 ** -24


def gamma(n, u=U):
    return n * u / (1 - n * u)


def cases(ri, ro):
    """the kernel test's inputs at (ri, ro): (length, content, samples)"""
    return list(exact_cases(ri, ro))


@pytest.mark.parametrize("ri,ro", MATRIX)
def test_model_within_the_error_bound_of_float64(built, ri, ro):
    """|fp32 chain - exact sum| <= gamma_2K sum |t x| (2K roundings, one per FMA); the float64 evaluation adds at most
    gamma64_2K sum |t x| (its products are exact).  An int16 output differs from sat16(rint(float64)) only where the float64 sum
    lies within that bound of a half-integer."""
    L, M, K, taps = A.resampler_taps(ri, ro)
    assert (L, M, K) == O.resample_lmk(ri, ro)
    checked = 0
    for n, kind, x in cases(ri, ro):
        y, acc, ab = O.resample(taps, ri, ro, x, acc=True)
        y64, acc64, _ = O.resample(taps, ri, ro, x, variant=4, acc=True)
        assert y.size == y64.size == (n * L + M - 1) // M
        bound = (gamma(2 * K) + gamma(2 * K, 2.0 ** -53)) * ab
        err = np.abs(acc - acc64)
        assert (err <= bound).all(), (n, kind, float((err - bound).max()))
        assert (y64 == np.clip(np.rint(acc64), -32768, 32767)).all()
        d = y != y64
        halfway = np.abs(acc64 - np.floor(acc64) - 0.5) <= bound
        assert (~d | halfway).all(), (n, kind, np.flatnonzero(d & ~halfway)[:8])
        checked += y.size
    assert checked > 0


def test_sensitivity_of_the_bit_exact_test(built):
    """mutants of the summation, on the bit-exact test's inputs: each changes at least one int16 output at every pair of the matrix
    and at least 10 summed over it"""
    names = {1: "reversed tap order", 2: "unfused multiply-add", 3: "two interleaved partial sums", 4: "float64 accumulator"}
    total = {v: 0 for v in names}
    for ri, ro in MATRIX:
        taps = A.resampler_taps(ri, ro)[3]
        per = {v: 0 for v in names}
        for n, kind, x in cases(ri, ro):
            y0 = O.resample(taps, ri, ro, x)
            for v in names:
                yv = O.resample(taps, ri, ro, x, variant=v)
                assert yv.size == y0.size
                per[v] += int((yv != y0).sum())
        print("%6d -> %5d Hz: outputs that differ from the contract: %s" % (ri, ro, ", ".join("%s %d" % (names[v], per[v]) for v in names)))
        for v in names:
            assert per[v] >= 1, (ri, ro, names[v])
            total[v] += per[v]
    for v in names:
        assert total[v] >= 10, (names[v], total[v])


def round_f32(q):
    """a Fraction rounded to the nearest float32, ties to even"""
    f = np.float32(float(q))
    cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    return min(cands, key=lambda c: (abs(Fraction(float(c)) - q), int(np.array(c).view(np.uint32)) & 1))


@pytest.mark.parametrize("ri,ro", [(48000, 16000), (44100, 16000), (8000, 44100)])
def test_model_is_the_contract_in_exact_arithmetic(built, ri, ro):
    """orc_resample against the contract restated in exact rational arithmetic: each step of the chain is the exact
    tap * x + acc rounded once to fp32 (an FMA), in increasing tap order, x = 0 outside the segment; then rint, saturation"""
    L, M, K, taps = A.resampler_taps(ri, ro)
    x = np.random.RandomState(3).randint(-32768, 32768, size=3 * K + 5).astype(np.int16)
    x[:K // 2] = 32767                                    # (a clamped stretch)
    y, acc, _ = O.resample(taps, ri, ro, x, acc=True)
    n_out = -(-x.size * L // M)
    assert y.size == n_out
    for j in range(0, n_out, max(1, n_out // 40)):
        k0, p = j * M // L, j * M % L
        a = np.float32(0.0)
        for i in range(2 * K):
            k = k0 - K + 1 + i
            xv = int(x[k]) if 0 <= k < x.size else 0
            a = round_f32(Fraction(float(taps[p, i])) * xv + Fraction(float(a)))
        assert a == np.float32(acc[j]), (j, a, acc[j])
        assert y[j] == int(np.clip(np.rint(a), -32768, 32767)), (j, a, y[j])


def lds_floats(L, M, K):
    """the kernel's LDS floats per block of 256 outputs (resample.h resample_lds_floats), restated"""
    return (255 * M + L - 1) // L + 1 + 2 * K + (2 * K if L == 1 else 0)


def test_plan_edges(built):
    from april_asr_amd import _ffi
    lmk = np.zeros(3, np.int32)
    # an 8 kHz model: 328000 Hz is the highest multiple of its rate whose block span fits 64 KB of LDS
    assert O.resample_lmk(328000, 8000) == (1, 41, 1458) and lds_floats(1, 41, 1458) == 16288
    assert A.resampler_taps(328000, 8000)[:3] == (1, 41, 1458)
    assert O.resample_lmk(336000, 8000) == (1, 42, 1494) and lds_floats(1, 42, 1494) == 16687
    assert _ffi.lib().aprilx_resampler_taps(336000, 8000, lmk.ctypes.data, None, 0) == -1
    # a 16 kHz model: 383996 Hz has the largest phase table accepted (L = 4000, 27 MB) and K = 854
    assert O.resample_lmk(383996, 16000) == (4000, 95999, 854) == A.resampler_taps(383996, 16000)[:3]
    assert lds_floats(4000, 95999, 854) <= 16384 and lds_floats(1, 24, 854) <= 16384
    # a 44.1 kHz model: 383996 Hz needs L = 11025 > 4096
    assert O.resample_lmk(383996, 44100)[0] == 11025
    assert _ffi.lib().aprilx_resampler_taps(383996, 44100, lmk.ctypes.data, None, 0) == -1
