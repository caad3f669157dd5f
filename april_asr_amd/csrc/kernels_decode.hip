// Decode of formatted sessions' input (kernels.h DecodeDesc, contract in input_format.h): G.711, float32, interleaved channels ->
// one int16 per audio frame, written into the staging buffer the resampler and the filterbank read.
//
// One workgroup of 256 lanes (4 waves of 64) per 256 consecutive outputs of one descriptor: grid (max blocks, descriptors), blocks
// past a descriptor's end leave at once.  Lane t decodes frame b0 + t: consecutive lanes read consecutive frames (G.711 mono: one
// byte each, F32 mono: one dword each) and write consecutive int16.  Every load is the aligned load of ONE value -- a byte, a
// 2-byte-aligned int16, a 4-byte-aligned binary32 (DecodeDesc's contract: spans start on 4-byte boundaries) -- never a wider one.
// G.711 is the closed form in integer ALU.  The pass moves a few MB at thousands of sessions and is bound by its launch, not by
// bandwidth: this is the plain form on purpose.
#include "kernels.h"

namespace aprilx {

namespace {

__device__ inline int dec_mulaw(unsigned b)
{
    const unsigned u = ~b & 0xFFu;
    const int mag = (int)(((((u & 15u) << 3) + 0x84u) << ((u >> 4) & 7u)) - 0x84u);
    return (u & 0x80u) ? -mag : mag;
}

__device__ inline int dec_alaw(unsigned b)
{
    const unsigned a = (b ^ 0x55u) & 0xFFu, e = (a >> 4) & 7u, m = a & 15u;
    const int mag = (int)(e == 0 ? (m << 4) + 8u : ((m << 4) + 0x108u) << (e - 1u));
    return (a & 0x80u) ? mag : -mag;
}

__device__ inline int dec_f32(float x)
{
    float y = x * 32768.0f;
    if (y != y) return 0;
    y = y < -32768.0f ? -32768.0f : (y > 32767.0f ? 32767.0f : y);
    return (int)__builtin_rintf(y);                    // round half to even (the default rounding mode)
}

// value `idx` (frame * channels + channel) of a span that starts at `p` (4-byte aligned)
__device__ inline int dec_value(int enc, const uint8_t *p, int64_t idx)
{
    switch (enc) {
    case 1: return dec_mulaw(p[idx]);
    case 2: return dec_alaw(p[idx]);
    case 3: return dec_f32(reinterpret_cast<const float *>(p)[idx]);
    default: return reinterpret_cast<const int16_t *>(p)[idx];
    }
}

}  // namespace

__global__ __launch_bounds__(kDecodeBlock) void decode_kernel(DecodeArgs a)
{
    const DecodeDesc d = a.desc[blockIdx.y];
    const int i = (int)blockIdx.x * kDecodeBlock + (int)threadIdx.x;
    if (i >= d.out_cnt) return;
    int v = 0;
    if (i < d.n_src) {
        const uint8_t *p = a.raw + d.src_off;
        const int C = d.channels;
        const int64_t f0 = (int64_t)i * C;
        if (d.channel >= 0) {
            v = dec_value(d.encoding, p, f0 + d.channel);
        } else {
            int s = 0;
            for (int c = 0; c < C; ++c) s += dec_value(d.encoding, p, f0 + c);
            const int n = 2 * s + C, q = 2 * C;
            v = n >= 0 ? n / q : -((-n + q - 1) / q);      // floor((2 S + C) / (2 C))
        }
    }
    a.out[(int64_t)d.dst + i] = (int16_t)v;
}

void launch_decode(const DecodeArgs &a, hipStream_t s)
{
    if (a.n_desc <= 0 || a.max_blocks <= 0) return;
    for (int d0 = 0; d0 < a.n_desc; d0 += 65535) {            // (grid.y limit)
        DecodeArgs b = a;
        b.desc = a.desc + d0;
        b.n_desc = a.n_desc - d0 < 65535 ? a.n_desc - d0 : 65535;
        hipLaunchKernelGGL(decode_kernel, dim3((unsigned)a.max_blocks, (unsigned)b.n_desc), dim3(kDecodeBlock), 0, s, b);
    }
}

}  // namespace aprilx
