// Line quality of opted-in sessions (kernels.h QualityDesc, contract in quality.h): per real frame of a session the sum, the sum of
// squares, minimum, maximum, clipped samples, longest clipped run and the dead flag of its hop -- the first H staged samples -- as one
// record of eight uint32.  Runs behind the decode and resample launches on the stream fbank_kernel runs on, on the samples fbank_kernel
// reads (FbankFrameDesc::pcm_off of the same pass).  Stateless: no per-slot record, no reset.  Integers only: the order of the fold is
// free and every bit is the host's.
//
// One wave per frame, four waves per workgroup.  The hop is walked in slabs of 64 samples, lane l taking sample 64 c + l of slab c
// (consecutive lanes read consecutive int16: one 128-byte line per slab); a lane behind the hop's end contributes nothing.  Sum, sum of
// squares (64 bits), minimum, maximum and the clip count fold over lane distances 32 .. 1 (__shfl_xor: no LDS, every lane holds the
// result).  clip_run is the one value that is no plain fold.  CHOICE: the per-lane clip flags of a slab go through a 64-bit ballot --
// bit l is sample 64 c + l, the same word in every lane --; the longest run of set bits inside the word is found by m &= m << 1 until
// the word is empty, and the slabs are joined in order by carrying the run that ends at the slab's last sample: a slab's leading run
// continues the carried one, and a slab that is all ones extends it.  (The alternative, lane 0 walking H flags from LDS, serialises H
// steps on one lane.)  All trip counts are the same for every lane of a wave, so all 64 lanes reach every shuffle and ballot.  Lane 0
// writes the record as two 16-byte stores.  Plain C++, vector loads and stores only, no atomics, no floating point.
#include "kernels.h"

namespace aprilx {

__global__ __launch_bounds__(kQualityBlock) void quality_kernel(QualityArgs a)
{
    const QualityDesc d = a.desc[blockIdx.x];
    const int lane = (int)threadIdx.x & (kQualityLanes - 1);
    const int waves = kQualityBlock / kQualityLanes;
    const int wave = (int)blockIdx.y * waves + ((int)threadIdx.x >> 6), stride = (int)gridDim.y * waves;
    const int H = a.hop, L = d.clip_level;
    if (wave >= d.n) return;                                   // (wave-uniform)

    for (int f = wave; f < d.n; f += stride) {
        const int pcm_off = a.frames[d.first + f].pcm_off;
        uint4 *o = reinterpret_cast<uint4 *>(a.out + (size_t)kQualityWords * ((size_t)d.out_off + (size_t)f));
        if (pcm_off < 0) {                                     // (cannot occur inside a run -- the host asserts it; never read in front of the buffer)
            if (lane == 0) { o[0] = make_uint4(0u, 0u, 0u, 0u); o[1] = make_uint4(0u, 0u, 0u, 0u); }
            continue;
        }
        const int16_t *x = a.pcm + pcm_off;
        unsigned long long sumsq = 0;
        int sum = 0, mn = 32767, mx = -32768, count = 0;
        int best = 0, carry = 0;                               // (the same in every lane)
        for (int j0 = 0; j0 < H; j0 += kQualityLanes) {
            const int j = j0 + lane;
            const bool in = j < H;
            const int v = in ? (int)x[j] : 0;
            const bool clip = in && (v >= L || v <= -L);
            if (in) {
                sumsq += (unsigned long long)(unsigned)(v * v);
                sum += v;
                mn = v < mn ? v : mn;
                mx = v > mx ? v : mx;
                count += clip ? 1 : 0;
            }
            const unsigned long long m = __ballot(clip);
            const int lead = ~m ? __builtin_ctzll(~m) : kQualityLanes;      // the run that starts at the slab's first sample
            const int joined = carry + lead;
            best = joined > best ? joined : best;
            int inside = 0;
            for (unsigned long long r = m; r; r &= r << 1) ++inside;        // longest run of set bits in the word
            best = inside > best ? inside : best;
            carry = ~m ? __builtin_clzll(~m) : carry + kQualityLanes;       // the run that ends at the slab's last sample
        }
#pragma unroll
        for (int k = kQualityLanes / 2; k >= 1; k >>= 1) {
            sumsq += __shfl_xor(sumsq, k);
            sum += __shfl_xor(sum, k);
            const int omn = __shfl_xor(mn, k), omx = __shfl_xor(mx, k);
            mn = omn < mn ? omn : mn;
            mx = omx > mx ? omx : mx;
            count += __shfl_xor(count, k);
        }
        if (lane == 0) {
            o[0] = make_uint4((unsigned)(sumsq & 0xffffffffull), (unsigned)(sumsq >> 32), (unsigned)sum, (unsigned)(mn & 0xffff) | (unsigned)(mx & 0xffff) << 16);
            o[1] = make_uint4(((unsigned)count & 0xffffu) | (unsigned)best << 16, mn == mx ? 1u : 0u, 0u, 0u);
        }
    }
}

void launch_quality(const QualityArgs &a, hipStream_t s)
{
    if (a.n_desc <= 0 || a.max_n <= 0 || a.hop <= 0) return;
    const int per_block = kQualityBlock / kQualityLanes * kQualityWaveFrames;
    int by = (a.max_n + per_block - 1) / per_block;
    if (by > kQualityMaxBlocks) by = kQualityMaxBlocks;
    hipLaunchKernelGGL(quality_kernel, dim3((unsigned)a.n_desc, (unsigned)by), dim3(kQualityBlock), 0, s, a);
}

}  // namespace aprilx
