// Voice activity of opted-in sessions (kernels.h VadDesc, contract in vad.h): per real frame of a session the band energy of its
// log-mel row, an exponential average over it, a running minimum as the noise floor, and a two-threshold state with onset and
// hangover counts -> one byte per frame.  Runs right behind fbank_kernel on the stream it ran on, on the rows it has just written.
//
// One workgroup of 256 lanes (4 waves of 64) per descriptor, in tiles of kVadTile frames:
//   phase 1  sixteen lanes per frame: lane l adds x[b0 + l + 16 k] in increasing k (consecutive lanes read consecutive floats of the
//            row), then the sixteen sums fold over lane distances 8, 4, 2, 1 inside their 16-lane group (__shfl_xor, width 16: no LDS)
//            -- the order of vad.h step 1, so every lane holds the host's bits -- and lane 0 of the group leaves e in LDS.  Sixteen
//            frames per pass of the workgroup; the trip count is the same for every lane, so all 64 lanes of a wave reach every shuffle.
//   phase 2  lane 0 walks the tile's energies through steps 2-9 with the state in registers (the eight sub-window minima are
//            written by compare-select, never through a computed index: nothing spills) and leaves the bytes in LDS;
//   then every lane stores one byte (consecutive lanes, consecutive bytes).
// A feed of 100 ms is 10 frames: one tile, one pass.  A minute fed at once is 6000 frames: 24 tiles, ~0.2 ms of one lane's serial walk.
// Plain C++, vector loads and stores only.  -ffp-contract=off (Makefile): t = 0.25f * t; s = s + t stays two roundings.
#include "kernels.h"

namespace aprilx {

namespace {

__device__ inline float dmin(float a, float b) { return b < a ? b : a; }
__device__ inline float dmax(float a, float b) { return a < b ? b : a; }

}  // namespace

__global__ __launch_bounds__(kVadBlock) void vad_kernel(VadArgs a)
{
    __shared__ float e_s[kVadTile];
    __shared__ uint8_t b_s[kVadTile];
    const VadDesc d = a.desc[blockIdx.x];
    const VadPlan p = d.plan;
    const int tid = (int)threadIdx.x, lane = tid & (kVadLanes - 1), grp = tid / kVadLanes;
    constexpr int kGroups = kVadBlock / kVadLanes;
    const float *ring = a.ring + (size_t)d.slot * (size_t)a.ring_frames * (size_t)a.nbins;
    const float inf = __builtin_inff();

    // (lane 0 only) the state: reset, or the slot's record
    float s = 0.0f, cur = inf, h[kVadSubWindows];
    int cnt = 0, pos = 0, st = 0, run = 0, first = 1;
#pragma unroll
    for (int i = 0; i < kVadSubWindows; ++i) h[i] = inf;
    if (tid == 0 && !(d.flags & VAD_RESET)) {
        const VadState v = a.state[d.slot];
        s = v.s; cur = v.cur; cnt = v.cnt; pos = v.pos; st = v.st; run = v.run; first = v.first;
#pragma unroll
        for (int i = 0; i < kVadSubWindows; ++i) h[i] = v.hist[i];
    }

    for (int f0 = 0; f0 < d.n; f0 += kVadTile) {
        const int nt = d.n - f0 < kVadTile ? d.n - f0 : kVadTile;
        const int passes = (nt + kGroups - 1) / kGroups;
        for (int it = 0; it < passes; ++it) {
            const int f = it * kGroups + grp;
            float c = 0.0f;
            if (f < nt) {
                int row = d.first_row + f0 + f;
                if (row >= a.ring_frames) row -= a.ring_frames;
                const float *x = ring + (size_t)row * (size_t)a.nbins;
                for (int i = p.b0 + lane; i < p.b1; i += kVadLanes) c = c + x[i];
            }
#pragma unroll
            for (int m = kVadLanes / 2; m >= 1; m >>= 1) c = c + __shfl_xor(c, m, kVadLanes);
            if (f < nt && lane == 0) e_s[f] = c * p.inv_nb;
        }
        __syncthreads();
        if (tid == 0) {
            for (int i = 0; i < nt; ++i) {
                float e = dmax(e_s[i], p.min_energy);
                if (first) { s = e; first = 0; }
                else { float t = e - s; t = kVadAlpha * t; s = s + t; }
                cur = dmin(cur, s); cnt += 1;
                float n = cur;
#pragma unroll
                for (int k = 0; k < kVadSubWindows; ++k) n = dmin(n, h[k]);
                const float dd = s - n;
                const int raw = dd > (st ? p.thr_off : p.thr_on) ? 1 : 0;
                if (cnt == kVadSubFrames) {
#pragma unroll
                    for (int k = 0; k < kVadSubWindows; ++k) h[k] = pos == k ? cur : h[k];
                    pos = (pos + 1) & (kVadSubWindows - 1); cur = inf; cnt = 0;
                }
                if (!st) { run = raw ? run + 1 : 0; if (run >= p.onset_frames) { st = 1; run = 0; } }
                else { run = raw ? 0 : run + 1; if (run >= p.hangover_frames) { st = 0; run = 0; } }
                b_s[i] = (uint8_t)(st | raw << 1);
            }
        }
        __syncthreads();
        if (tid < nt) {
            const size_t o = (size_t)d.out_off + (size_t)f0 + (size_t)tid;
            a.out[o] = b_s[tid];
            if (a.energy) a.energy[o] = e_s[tid];
        }
        __syncthreads();                                       // (the next tile overwrites e_s / b_s)
    }
    if (tid == 0) {
        VadState v;
        v.s = s; v.cur = cur; v.cnt = cnt; v.pos = pos; v.st = st; v.run = run; v.first = first; v.reserved = 0;
#pragma unroll
        for (int i = 0; i < kVadSubWindows; ++i) v.hist[i] = h[i];
        a.state[d.slot] = v;
    }
}

void launch_vad(const VadArgs &a, hipStream_t s)
{
    if (a.n_desc <= 0) return;
    hipLaunchKernelGGL(vad_kernel, dim3((unsigned)a.n_desc), dim3(kVadBlock), 0, s, a);
}

}  // namespace aprilx
