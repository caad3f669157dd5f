// Tones of opted-in sessions (kernels.h ToneDesc, contract in tone.h): per real frame of a session the correlation of its first W staged
// samples with cos and sin of every bin of the grid (2F table rows of W values: 65 536 multiply-adds per frame at 16 kHz, sixteen times
// dtmf_kernel's), the frame's energy, and the decision of tone.h steps 3-7 -> one record of two uint16 per frame.  Runs beside
// dtmf_kernel on the stream fbank_kernel runs on, on the samples fbank_kernel reads.  Stateless: no per-slot record, no reset.
//
// One wave per workgroup, G = kToneWaveFrames consecutive frames of one run per wave.  Lane l owns chain l -- samples l, l + 64, ... of
// every frame, multiply then add in increasing index, the order of tone.h step 1.  The tables (256 KiB at W = 512) fit neither registers
// nor LDS whole, so the SAMPLES stay put and the tables stream: a lane keeps its W / 64 samples of the G frames as floats in registers
// (W <= 512: NC = W / 64 <= 8, 32 registers; beyond that, NC = 0 below, they are re-read per walk from L1) and walks the rows
// kToneBins bins at a time -- 8 bins x {cos, sin} x G frames = 64 chain sums per lane.  Every table element is read once per G frames,
// consecutive lanes reading consecutive floats of a table that stays in L2: 2 F W 4 / G bytes per frame, 64 KiB at 16 kHz.
//
// The fold a[l] = a[l] + a[l ^ m], m = 32 .. 1, is done on the 64 sums of a walk TOGETHER: at distance m a lane with bit m set keeps
// the upper m of its 2 m sums and sends the lower ones, its partner the reverse, so each step halves what a lane holds and after six
// steps lane i holds the complete sum of item i -- 63 shuffles per walk instead of 384.  A lane adds exactly the two values the plain
// fold adds at that step (IEEE addition commutes), so the bits are the contract's.  Items are ordered (bin, frame, cos | sin): re and im
// of a frame's bin land in lanes 2 j and 2 j + 1, one more shuffle gives P, which goes to a row of LDS per frame.  The integer energy
// (exact in 64 bits, so its order is free) folds the plain way.  Lanes 0 .. G - 1 then each run the ONE tone_decide (shared with the host
// and with tone_decide_kernel) on a frame's row and store its four bytes.  All trip counts are the same for every lane of the wave:
// all 64 lanes reach every shuffle and both barriers.  A padding row (pcm_off < 0; cannot occur inside a run) or a frame behind the
// run's end is never read.  Plain C++, vector loads and stores only.  -ffp-contract=off (Makefile): the chains and re * re + im * im
// stay multiply-then-add.
#include "kernels.h"

namespace aprilx {

constexpr int kToneMaxBlocks = 64;      // workgroups per descriptor; a longer run is walked in strides

template <int NC> __global__ __launch_bounds__(kToneBlock) void tone_kernel(ToneArgs a)
{
    constexpr int G = kToneWaveFrames, B = kToneBins, ITEMS = B * G * 2;
    static_assert(ITEMS == kToneLanes, "one item per lane after the fold");
    __shared__ float Pl[G][kToneMaxF + 1];                     // P[0..F) and E of the wave's frames
    const ToneDesc d = a.desc[blockIdx.x];
    const int lane = (int)threadIdx.x;
    const int w = a.w, F = a.f;
    const int nc = NC > 0 ? NC : w / kToneLanes;

    for (int f0 = (int)blockIdx.y * G; f0 < d.n; f0 += (int)gridDim.y * G) {      // (uniform)
        const int16_t *x[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int pcm_off = f0 + g < d.n ? a.frames[d.first + f0 + g].pcm_off : -1;
            x[g] = pcm_off >= 0 ? a.pcm + pcm_off : nullptr;
        }
        float xr[G][NC > 0 ? NC : 1];
        long long e[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            e[g] = 0;
            if (NC > 0) {
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const int xi = x[g] ? (int)x[g][lane + kToneLanes * c] : 0;
                    xr[g][c] = (float)xi;
                    e[g] += (long long)(xi * xi);
                }
            } else if (x[g]) {
                for (int c = 0; c < nc; ++c) { const int xi = (int)x[g][lane + kToneLanes * c]; e[g] += (long long)(xi * xi); }
            }
        }

        for (int k0 = 0; k0 < F; k0 += B) {
            float acc[ITEMS];
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) acc[i] = 0.0f;
            int row[B];                                        // (bins behind the grid's end repeat its last bin; their sums are dropped)
#pragma unroll
            for (int b = 0; b < B; ++b) row[b] = (k0 + b < F ? k0 + b : F - 1) * w + lane;
            const float *tc = a.tables, *ts = a.tables + F * w;
            auto link = [&](int c, const float *xv) {
#pragma unroll
                for (int b = 0; b < B; ++b) {
                    const float vc = tc[row[b] + kToneLanes * c], vs = ts[row[b] + kToneLanes * c];
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        const float mc = xv[g] * vc; acc[(b * G + g) * 2] = acc[(b * G + g) * 2] + mc;
                        const float ms = xv[g] * vs; acc[(b * G + g) * 2 + 1] = acc[(b * G + g) * 2 + 1] + ms;
                    }
                }
            };
            if (NC > 0) {
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    float xv[G];
#pragma unroll
                    for (int g = 0; g < G; ++g) xv[g] = xr[g][c];
                    link(c, xv);
                }
            } else {
                for (int c = 0; c < nc; ++c) {
                    float xv[G];
#pragma unroll
                    for (int g = 0; g < G; ++g) xv[g] = x[g] ? (float)(int)x[g][lane + kToneLanes * c] : 0.0f;
                    link(c, xv);
                }
            }
#pragma unroll
            for (int m = kToneLanes / 2; m >= 1; m >>= 1) {
                const bool up = (lane & m) != 0;
#pragma unroll
                for (int i = 0; i < m; ++i) {
                    const float keep = up ? acc[i + m] : acc[i], send = up ? acc[i] : acc[i + m];
                    acc[i] = keep + __shfl_xor(send, m);
                }
            }
            const float sq = acc[0] * acc[0];                  // lane = item: (bin lane / 8, frame (lane / 2) % 4, cos | sin)
            const float pw = sq + __shfl_xor(sq, 1);
            const int b = lane / (2 * G), g = (lane >> 1) & (G - 1);
            if (!(lane & 1) && k0 + b < F) Pl[g][k0 + b] = pw;
        }
#pragma unroll
        for (int m = kToneLanes / 2; m >= 1; m >>= 1) {
#pragma unroll
            for (int g = 0; g < G; ++g) e[g] += __shfl_xor(e[g], m);
        }
        if (lane == 0) {
#pragma unroll
            for (int g = 0; g < G; ++g) Pl[g][F] = (float)e[g];
        }
        __syncthreads();
        if (lane < G && f0 + lane < d.n) {
            const bool real = a.frames[d.first + f0 + lane].pcm_off >= 0;
            const size_t o = (size_t)d.out_off + (size_t)(f0 + lane);
            const float *P = Pl[lane];
            a.out[o] = real ? tone_decide(d.plan, P, P[F]) : 0u;
            if (a.powers) for (int k = 0; k <= F; ++k) a.powers[o * (size_t)(F + 1) + (size_t)k] = real ? P[k] : 0.0f;
        }
        __syncthreads();                                       // (the next group of frames overwrites the rows)
    }
}

__global__ __launch_bounds__(256) void tone_decide_kernel(TonePlan p, int n, const float *powers, uint32_t *records_out)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const float *P = powers + (size_t)i * (size_t)(p.F + 1);
    records_out[i] = tone_decide(p, P, P[p.F]);
}

void launch_tone(const ToneArgs &a, hipStream_t s)
{
    if (a.n_desc <= 0 || a.max_n <= 0) return;
    int by = (a.max_n + kToneWaveFrames - 1) / kToneWaveFrames;
    if (by > kToneMaxBlocks) by = kToneMaxBlocks;
    const dim3 grid((unsigned)a.n_desc, (unsigned)by), block(kToneBlock);
    switch (a.w) {
    case 256: hipLaunchKernelGGL(tone_kernel<4>, grid, block, 0, s, a); break;
    case 384: hipLaunchKernelGGL(tone_kernel<6>, grid, block, 0, s, a); break;
    case 512: hipLaunchKernelGGL(tone_kernel<8>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(tone_kernel<0>, grid, block, 0, s, a); break;
    }
}

void launch_tone_decide(const TonePlan &plan, int n, const float *powers, uint32_t *records_out, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(tone_decide_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, plan, n, powers, records_out);
}

}  // namespace aprilx
