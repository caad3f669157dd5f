// aprilx_run_conv_front / aprilx_conv_front_geometry (include/aprilx_engine.h): ONE launch of the conv front end against host arrays,
// for tests/test_gpu_conv_front.py.  The weights are transposed by launch_conv_weight_transpose into one allocation, as Engine::load
// does, the launch is launch_conv_embed with the engine's argument block (Engine::encoder_front).  No rule is restated here: the
// geometry, the channels per workgroup and the refusal come from conv_front.h, the form from conv_embed_form.
#include <hip/hip_runtime.h>
#include <cstring>
#include <string>
#include "../../include/aprilx_engine.h"
#include "common.h"
#include "kernels.h"
#include "debug_arena.h"

using namespace aprilx;

namespace {

enum { D_SEG, D_MEL, D_S0, D_S1, D_S2, D_C0, D_C1, D_M, D_LDO, D_OUT_ROWS, D_SLOTS, D_RING_FRAMES };
enum { I_W0, I_B0, I_W1, I_B1, I_X, I_RING, I_SLOT, I_TAIL };
enum { O_OUT, O_W0T, O_W1T };

// the argument block without pointers, and what the host knows about it; false = not to be launched
bool describe(const int32_t *d, ConvEmbedArgs &ca, ConvFrontGeom &g, int32_t *info)
{
    ca.seg = d[D_SEG]; ca.mel = d[D_MEL]; ca.M = d[D_M]; ca.ldo = d[D_LDO]; ca.ring_frames = d[D_RING_FRAMES];
    for (int i = 0; i < 3; ++i) ca.stride[i] = d[D_S0 + i];
    ca.ch[0] = d[D_C0]; ca.ch[1] = d[D_C1];
    std::string why;
    const bool ok = conv_front_ok(ca.seg, ca.mel, ca.stride, ca.ch[0], ca.ch[1], why);
    g = conv_front_geom(ca.seg, ca.mel, ca.stride, ca.ch[0], ca.ch[1]);
    ca.ch1_per_group = g.cg;
    const int32_t r[12] = {g.H1, g.W1, g.H2, g.W2, g.W3, g.NP, g.cg, (int32_t)(g.lds_bytes > 0x7fffffff ? 0x7fffffff : g.lds_bytes), 0, ok ? 1 : 0, 0, 0};
    std::memcpy(info, r, sizeof r);
    if (!ok) return false;
    // sizes a launch could not be made with, or that would write outside the arrays
    if (ca.M < 1 || ca.M > (1 << 16) || ca.ch[0] > 4096 || ca.ch[1] > 4096 || ca.ldo < 9 * ca.ch[1] || (long)d[D_OUT_ROWS] < (long)ca.M * g.W3 ||
        ca.ring_frames < ca.seg || d[D_SLOTS] < 0) { info[9] = 0; return false; }
    return true;
}

}  // namespace

extern "C" int aprilx_conv_front_geometry(const int32_t *d, int32_t *info)
{
    if (!d || !info) return -1;
    ConvEmbedArgs ca; ConvFrontGeom g;
    if (!describe(d, ca, g, info)) return -1;
    static const float present = 0.0f;                   // the form does not depend on the weights, only on their being there
    ca.w0t = ca.w1t = &present;
    info[8] = conv_embed_form(ca);
    return 0;
}

extern "C" int aprilx_run_conv_front(const int32_t *d, const void *const *in, void *const *out, int32_t *info)
{
    if (!d || !in || !out || !info) return -1;
    ConvEmbedArgs ca; ConvFrontGeom g;
    if (!describe(d, ca, g, info)) return -1;
    const size_t M = (size_t)ca.M, c0 = (size_t)ca.ch[0], c1 = (size_t)ca.ch[1], chunk = (size_t)ca.seg * ca.mel, S = (size_t)d[D_SLOTS];
    if (!in[I_W0] || !in[I_B0] || !in[I_W1] || !in[I_B1] || !out[O_OUT]) return -1;
    if (S == 0 ? !in[I_X] : (!in[I_RING] || !in[I_SLOT] || !in[I_TAIL])) return -1;
    if (S) {
        const int32_t *slot = (const int32_t *)in[I_SLOT], *tail = (const int32_t *)in[I_TAIL];
        for (size_t m = 0; m < M; ++m) if (slot[m] < 0 || (size_t)slot[m] >= S || tail[m] < 0 || tail[m] >= ca.ring_frames) return -1;
    }

    Arena A("aprilx_run_conv_front");
    hipStream_t st = nullptr;
    ca.w[0] = (const float *)A.upload(in[I_W0], c0 * 9 * 4, c0 * 9 * 4); ca.b[0] = (const float *)A.upload(in[I_B0], c0 * 4, c0 * 4);
    ca.w[1] = (const float *)A.upload(in[I_W1], c1 * c0 * 9 * 4, c1 * c0 * 9 * 4); ca.b[1] = (const float *)A.upload(in[I_B1], c1 * 4, c1 * 4);
    if (S) {
        ca.ring = (const float *)A.upload(in[I_RING], S * ca.ring_frames * ca.mel * 4, 0);
        ca.slot_idx = (const int *)A.upload(in[I_SLOT], M * 4, 0); ca.ring_tail = (const int *)A.upload(in[I_TAIL], M * 4, 0);
    } else {
        ca.x_direct = (const float *)A.upload(in[I_X], M * chunk * 4, 0);
    }
    float *wt = (float *)A.raw((9 * c0 + 9 * c0 * c1) * 4, 0xFF);                 // [9][c0] then [c0 * 9][c1]: one allocation, as the engine keeps them
    const size_t out_bytes = (size_t)d[D_OUT_ROWS] * ca.ldo * 4;
    ca.out = (float *)A.raw(out_bytes, 0xFF);
    if (A.bad) return -2;
    ca.w0t = wt; ca.w1t = wt + 9 * c0;
    info[8] = conv_embed_form(ca);

    launch_conv_weight_transpose(ca.w[0], ca.w[1], ca.ch[0], ca.ch[1], wt, wt + 9 * c0, st);
    launch_conv_embed(ca, st);
    if (!A.ok(hipGetLastError()) || !A.ok(hipDeviceSynchronize())) return -2;

    A.download(out[O_OUT], ca.out, out_bytes);
    A.download(out[O_W0T], ca.w0t, 9 * c0 * 4);
    A.download(out[O_W1T], ca.w1t, 9 * c0 * c1 * 4);
    return A.bad ? -2 : 0;
}
