/*
 * ORACLE (test infrastructure, NOT product code): the input sample-rate conversion's contract (DESIGN.md section 11,
 * april_asr_amd/csrc/resample.h) evaluated on the CPU for one whole segment:
 *
 *   y[j] = sat16(round_half_even(sum_i tap[p][i] x[k0 - K + 1 + i])),  k0 = floor(j M / L),  p = j M mod L,  j < ceil(n L / M),
 *
 * the sum ONE fp32 FMA chain (fmaf) in increasing i, x = 0 outside the segment.  The library exports the phase table
 * (aprilx_resampler_taps, checked against the float64 formula by tests/test_resample_cpu.py); this file only applies it.
 * Built with -ffp-contract=off -fno-fast-math (oracle/Makefile): the compiler neither fuses nor reorders the variants below.
 *
 * `variant` is for tests only (tests/test_resample_oracle.py): the ways a kernel could sum differently, to show that a bit-exact
 * comparison with variant 0 tells each of them apart.
 */
#include <math.h>
#include "orc.h"

static float orc_rs_x(const int16_t *x, int64_t n, int64_t k) { return (k >= 0 && k < n) ? (float)x[k] : 0.0f; }

int64_t orc_resample(const float *taps, int L, int M, int K, int ldt, const int16_t *x, int64_t n, int variant,
                     int16_t *y, double *acc_out, double *abs_out)
{
    if (L < 1 || M < 1 || K < 0 || ldt < 2 * K || n < 0 || variant < 0 || variant > 4) return -1;
    const int64_t n_out = (n * L + M - 1) / M;
    const int t = 2 * K;
    for (int64_t j = 0; j < n_out; ++j) {
        const int64_t k0 = j * M / L;
        const int p = (int)(j * M - k0 * L);
        const float *row = taps + (size_t)p * (size_t)ldt;
        const int64_t kb = k0 - K + 1;
        double acc;
        if (variant == 0) {                          /* the contract */
            float a = 0.0f;
            for (int i = 0; i < t; ++i) a = fmaf(row[i], orc_rs_x(x, n, kb + i), a);
            acc = a;
        } else if (variant == 1) {                   /* reversed tap order */
            float a = 0.0f;
            for (int i = t - 1; i >= 0; --i) a = fmaf(row[i], orc_rs_x(x, n, kb + i), a);
            acc = a;
        } else if (variant == 2) {                   /* unfused: the product rounded to fp32, then added */
            float a = 0.0f;
            for (int i = 0; i < t; ++i) {
                const float pr = row[i] * orc_rs_x(x, n, kb + i);
                a = a + pr;
            }
            acc = a;
        } else if (variant == 3) {                   /* two interleaved partial sums (even / odd taps), added at the end */
            float a0 = 0.0f, a1 = 0.0f;
            for (int i = 0; i < t; i += 2) {         /* (t = 2K is even) */
                a0 = fmaf(row[i], orc_rs_x(x, n, kb + i), a0);
                a1 = fmaf(row[i + 1], orc_rs_x(x, n, kb + i + 1), a1);
            }
            acc = (double)(a0 + a1);
        } else {                                     /* float64 accumulator (each product is exact in double) */
            double a = 0.0;
            for (int i = 0; i < t; ++i) a += (double)row[i] * (double)orc_rs_x(x, n, kb + i);
            acc = a;
        }
        if (acc_out) acc_out[j] = acc;
        if (abs_out) {
            double s = 0.0;
            for (int i = 0; i < t; ++i) s += fabs((double)row[i] * (double)orc_rs_x(x, n, kb + i));
            abs_out[j] = s;
        }
        if (y) {
            /* variants 0-3: acc holds an fp32 value, rintf of it is the fp32 rounding; variant 4 rounds the double */
            double r = variant == 4 ? rint(acc) : (double)rintf((float)acc);
            r = r < -32768.0 ? -32768.0 : (r > 32767.0 ? 32767.0 : r);
            y[j] = (int16_t)r;
        }
    }
    return n_out;
}
