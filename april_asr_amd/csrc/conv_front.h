// Geometry of the conv front end (kernels_misc.hip conv12_kernel / conv12_wide_kernel), stated once on the host: the sizes after each
// convolution, the second conv's channels per workgroup, the dynamic shared memory of a workgroup and which geometries can be launched.
// Used by the loader (model_loader.cc extract_encoder), the blob import (april_api.cc), launch_conv_embed, Engine::encoder_front and
// the test entry aprilx_run_conv_front (conv_debug_api.cc).  No HIP here.
#pragma once
#include <cstddef>
#include <string>
#include "model_loader.h"

namespace aprilx {

// what a workgroup may ask for without raising the kernel's limit (hipFuncAttributeMaxDynamicSharedMemorySize is not raised for these kernels)
constexpr size_t CONV_FRONT_LDS_LIMIT = 64 * 1024;

// second-conv channels per workgroup of the grouped form: the largest divisor of the channel count that is <= 8 (a thread holds
// at most 8 accumulators)
inline int conv_ch1_per_group(int c1)
{
    for (int k = 8; k > 1; --k) if (c1 % k == 0) return k;
    return 1;
}

struct ConvFrontGeom {
    int H1 = 0, W1 = 0, H2 = 0, W2 = 0, H3 = 0, W3 = 0;      // rows x columns after conv 1, 2, 3 (3 x 3 kernels, no padding)
    int NP = 0;                                               // positions of the second conv: H2 * W2
    int cg = 0;                                               // conv_ch1_per_group
    size_t lds_bytes = 0;                                     // grouped form: the chunk, conv 1's output, one channel group of conv 2's
    bool valid = false;                                       // every conv sees at least 3 x 3 and the stack ends on one row
};

inline ConvFrontGeom conv_front_geom(int seg, int mel, const int stride[3], int c0, int c1)
{
    ConvFrontGeom g;
    if (seg < 3 || mel < 3 || stride[0] < 1 || stride[1] < 1 || stride[2] < 1 || c0 < 1 || c1 < 1) return g;
    g.H1 = (seg - 3) / stride[0] + 1; g.W1 = (mel - 3) / stride[0] + 1;
    if (g.H1 < 3 || g.W1 < 3) return g;
    g.H2 = (g.H1 - 3) / stride[1] + 1; g.W2 = (g.W1 - 3) / stride[1] + 1;
    if (g.H2 < 3 || g.W2 < 3) return g;
    g.H3 = (g.H2 - 3) / stride[2] + 1; g.W3 = (g.W2 - 3) / stride[2] + 1;
    g.NP = g.H2 * g.W2;
    g.cg = conv_ch1_per_group(c1);
    g.lds_bytes = sizeof(float) * ((size_t)seg * mel + (size_t)c0 * g.H1 * g.W1 + (size_t)g.cg * g.NP);
    g.valid = g.H3 == 1;
    return g;
}
inline ConvFrontGeom conv_front_geom(const NetDims &d) { return conv_front_geom(d.seg, d.mel, d.conv_stride, d.conv_ch[0], d.conv_ch[1]); }

// Can the front end run this network?  False with a message that names the geometry: a conv that sees fewer than 3 rows or columns,
// a stack that does not end on one frame, or more shared memory per workgroup than a launch gets.
inline bool conv_front_ok(int seg, int mel, const int stride[3], int c0, int c1, std::string &why)
{
    const ConvFrontGeom g = conv_front_geom(seg, mel, stride, c0, c1);
    const std::string shape = "conv front end (segment " + std::to_string(seg) + ", mel " + std::to_string(mel) + ", strides " + std::to_string(stride[0]) + "," +
                              std::to_string(stride[1]) + "," + std::to_string(stride[2]) + ", channels " + std::to_string(c0) + "," + std::to_string(c1) + "): ";
    if (!g.valid) {
        why = shape + (g.H3 > 1 ? "the stack must reduce the segment to one frame (got " + std::to_string(g.H3) + ")"
                                : std::string("every 3x3 convolution needs at least 3 rows and 3 columns of input"));
        return false;
    }
    if (g.lds_bytes > CONV_FRONT_LDS_LIMIT) {
        why = shape + "needs " + std::to_string(g.lds_bytes) + " bytes of shared memory per workgroup, more than the " + std::to_string(CONV_FRONT_LDS_LIMIT) + " a launch gets";
        return false;
    }
    return true;
}
inline bool conv_front_ok(const NetDims &d, std::string &why) { return conv_front_ok(d.seg, d.mel, d.conv_stride, d.conv_ch[0], d.conv_ch[1], why); }

}  // namespace aprilx
