// DTMF digits of opted-in sessions (kernels.h DtmfDesc, contract in dtmf.h): per real frame of a session the correlation of its first
// Wd staged samples with cos and sin of the eight DTMF frequencies, the frame's energy, and the decision of dtmf.h steps 3-4 -> one byte
// per frame.  Runs behind the decode and resample launches on the stream fbank_kernel runs on, on the samples fbank_kernel reads
// (FbankFrameDesc::pcm_off of the same pass).  Stateless: no per-slot record, no reset.
//
// One wave per frame.  Lane l owns chain l of all 16 table rows -- samples l, l + 64, ... below Wd, multiply then add in increasing
// index, the order of dtmf.h step 1 -- and the integer energy of the same samples (exact in 64 bits, so its order is free).  The 16
// sums and the energy fold over lane distances 32, 16, 8, 4, 2, 1 (__shfl_xor: no LDS, every lane holds the host's bits); lane 0 decides
// (dtmf_decide, the ONE statement of steps 3-4, shared with the host and with dtmf_decide_kernel) and stores the byte.  Consecutive
// lanes read consecutive int16: one 128-byte line per chain step.
//
// Table values: a lane's 16 x ceil(Wd / 64) values are the same for every frame.  CHOICE: for Wd <= 256 (NC = ceil(Wd / 64) <= 4:
// every model at 8 or 16 kHz) they are loaded ONCE per wave into registers (64 floats at Wd = 256) and kept across the frames the wave
// walks; for a larger Wd (NC = 0 below) they are read from global memory per frame, where consecutive lanes read consecutive floats of a
// table that stays in L2 -- at most 256 KiB at Wd = 4096, more than LDS holds, which is why LDS is not used.
// A 100 ms feed is 10 frames per session: one workgroup, waves of 3, 3, 2, 2 frames.  The trip counts are the same for every lane of a
// wave, so all 64 lanes reach every shuffle.  Plain C++, vector loads and stores only.  -ffp-contract=off (Makefile): the chains and
// re * re + im * im stay multiply-then-add.
#include "kernels.h"

namespace aprilx {

template <int NC> __global__ __launch_bounds__(kDtmfBlock) void dtmf_kernel(DtmfArgs a)
{
    const DtmfDesc d = a.desc[blockIdx.x];
    const DtmfPlan p = d.plan;
    const int lane = (int)threadIdx.x & (kDtmfLanes - 1);
    const int waves = kDtmfBlock / kDtmfLanes;
    const int wave = (int)blockIdx.y * waves + ((int)threadIdx.x >> 6), stride = (int)gridDim.y * waves;
    const int wd = a.wd;
    if (wave >= d.n) return;                                   // (wave-uniform)

    float T[kDtmfRows][NC > 0 ? NC : 1];
    if (NC > 0) {
#pragma unroll
        for (int r = 0; r < kDtmfRows; ++r)
#pragma unroll
            for (int k = 0; k < NC; ++k) { const int j = lane + kDtmfLanes * k; T[r][k] = j < wd ? a.tables[(size_t)r * (size_t)wd + (size_t)j] : 0.0f; }
    }

    for (int f = wave; f < d.n; f += stride) {
        const int pcm_off = a.frames[d.first + f].pcm_off;
        const size_t o = (size_t)d.out_off + (size_t)f;
        if (pcm_off < 0) {                                     // (cannot occur inside a run -- the host asserts it; never read in front of the buffer)
            if (lane == 0) { a.out[o] = 0; if (a.powers) for (int k = 0; k < 9; ++k) a.powers[o * 9 + (size_t)k] = 0.0f; }
            continue;
        }
        const int16_t *x = a.pcm + pcm_off;
        float acc[kDtmfRows];
#pragma unroll
        for (int r = 0; r < kDtmfRows; ++r) acc[r] = 0.0f;
        long long e = 0;
        if (NC > 0) {
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                const int j = lane + kDtmfLanes * k;
                if (j < wd) {
                    const int xi = (int)x[j];
                    const float xv = (float)xi;
                    e += (long long)(xi * xi);
#pragma unroll
                    for (int r = 0; r < kDtmfRows; ++r) { const float m = xv * T[r][k]; acc[r] = acc[r] + m; }
                }
            }
        } else {
            for (int j = lane; j < wd; j += kDtmfLanes) {
                const int xi = (int)x[j];
                const float xv = (float)xi;
                e += (long long)(xi * xi);
#pragma unroll
                for (int r = 0; r < kDtmfRows; ++r) { const float m = xv * a.tables[(size_t)r * (size_t)wd + (size_t)j]; acc[r] = acc[r] + m; }
            }
        }
#pragma unroll
        for (int m = kDtmfLanes / 2; m >= 1; m >>= 1) {
#pragma unroll
            for (int r = 0; r < kDtmfRows; ++r) acc[r] = acc[r] + __shfl_xor(acc[r], m);
            e += __shfl_xor(e, m);
        }
        if (lane == 0) {
            float q[9];
#pragma unroll
            for (int k = 0; k < 8; ++k) { const float rr = acc[k] * acc[k], ii = acc[8 + k] * acc[8 + k]; q[k] = rr + ii; }
            q[8] = (float)e;
            a.out[o] = (uint8_t)dtmf_decide(p, q, q[8]);
            if (a.powers) {
#pragma unroll
                for (int k = 0; k < 9; ++k) a.powers[o * 9 + (size_t)k] = q[k];
            }
        }
    }
}

__global__ __launch_bounds__(256) void dtmf_decide_kernel(DtmfPlan p, int n, const float *powers9, uint8_t *codes_out)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    float q[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) q[k] = powers9[(size_t)i * 9 + (size_t)k];
    codes_out[i] = (uint8_t)dtmf_decide(p, q, q[8]);
}

void launch_dtmf(const DtmfArgs &a, hipStream_t s)
{
    if (a.n_desc <= 0 || a.max_n <= 0) return;
    const int per_block = kDtmfBlock / kDtmfLanes * kDtmfWaveFrames;
    int by = (a.max_n + per_block - 1) / per_block;
    if (by > kDtmfMaxBlocks) by = kDtmfMaxBlocks;
    const dim3 grid((unsigned)a.n_desc, (unsigned)by), block(kDtmfBlock);
    switch (a.wd <= 4 * kDtmfLanes ? (a.wd + kDtmfLanes - 1) / kDtmfLanes : 0) {
    case 1: hipLaunchKernelGGL(dtmf_kernel<1>, grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL(dtmf_kernel<2>, grid, block, 0, s, a); break;
    case 3: hipLaunchKernelGGL(dtmf_kernel<3>, grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL(dtmf_kernel<4>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(dtmf_kernel<0>, grid, block, 0, s, a); break;
    }
}

void launch_dtmf_decide(const DtmfPlan &plan, int n, const float *powers9, uint8_t *codes_out, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(dtmf_decide_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, plan, n, powers9, codes_out);
}

}  // namespace aprilx
