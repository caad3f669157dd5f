// Session snapshot / restore, the device half: ONE launch gathers the per-slot state of n sessions -- the rows of
// h, c, h16, eout, dout, the search state, the trie state, the VAD state and the ring rows the session's book can still name -- into one
// device block per session in a staging buffer, or scatters such blocks back into the slots of n fresh sessions.  Memory-bound and
// nothing else: a lane moves 16 bytes per access (4 where a base, a stride or a width is no multiple of 16), consecutive lanes move
// consecutive bytes of the block and, inside a row, consecutive bytes of the array, so both sides are coalesced; blockIdx.y is the
// session, blockIdx.x strides over its block.  The hosts check slots, row counts and tails before the launch: the kernel trusts them.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "kernels.h"

namespace aprilx {

namespace {
__device__ inline void set_zero(uint4 &v) { v = make_uint4(0u, 0u, 0u, 0u); }
__device__ inline void set_zero(uint32_t &v) { v = 0u; }

template <typename V> __global__ __launch_bounds__(256) void snapshot_copy_kernel(SnapArgs a)
{
    const SnapRec r = a.recs[blockIdx.y];
    char *blk = a.stage + r.stage_off;
    const uint32_t units = r.block_bytes / (uint32_t)sizeof(V);
    for (uint32_t u = blockIdx.x * 256u + threadIdx.x; u < units; u += gridDim.x * 256u) {
        const uint32_t o = u * (uint32_t)sizeof(V);
        char *p = nullptr;                               // where byte o of the block lives in the engine's arrays; null: padding or an array the session leaves out
        bool word = false;                               // a one-word row (the trie state) under 16-byte accesses: only its 4 bytes are the array's
        for (int i = 0; i < a.n_arr; ++i) {
            const SnapArray &d = a.arr[i];
            const uint32_t rows = d.ring ? (uint32_t)r.rows : d.layers;
            if (o < d.off || o - d.off >= rows * d.row_bytes) continue;
            if (((r.mask >> i) & 1u) && d.base) {
                uint32_t row = (o - d.off) / d.row_bytes;
                const uint32_t col = (o - d.off) - row * d.row_bytes;
                if (d.ring) row = (uint32_t)(((a.scatter ? r.tgt_tail : r.tail) + (int)row) % a.ring_frames);
                p = d.base + (size_t)r.slot * d.slot_stride + (size_t)row * d.layer_stride + col;
                word = sizeof(V) > 4 && d.row_bytes == 4;
            }
            break;
        }
        V *s = reinterpret_cast<V *>(blk + o);
        if (word) {
            uint32_t *sw = reinterpret_cast<uint32_t *>(blk + o), *pw = reinterpret_cast<uint32_t *>(p);
            if (a.scatter) *pw = *sw;
            else { V v; set_zero(v); *s = v; *sw = *pw; }
        } else if (a.scatter) {
            if (p) *reinterpret_cast<V *>(p) = *s;
        } else {
            V v;
            if (p) v = *reinterpret_cast<const V *>(p); else set_zero(v);
            *s = v;
        }
    }
}
}  // namespace

void launch_snapshot_copy(const SnapArgs &a, hipStream_t s)
{
    if (a.n <= 0 || a.max_block == 0) return;
    const unsigned per = (unsigned)a.vec * 256u;
    // (a full GPU is n in the thousands: a few workgroups per session are enough to fill it, and one session alone still gets several)
    const unsigned bx = std::max(1u, std::min((a.max_block + per - 1) / per, a.n >= 256 ? 4u : 32u));
    const dim3 grid(bx, (unsigned)a.n);
    if (a.vec == 16) hipLaunchKernelGGL(snapshot_copy_kernel<uint4>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(snapshot_copy_kernel<uint32_t>, grid, dim3(256), 0, s, a);
}

}  // namespace aprilx
