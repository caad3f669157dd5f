// A row-epilogue GEMM given in its fused form (EPI_HR / EPI_RESID_SSQ / EPI_SLOT_STORE): the partial-plane form of the same GEMM
// over the workspace rows of its output, and the row problem that finishes it (same arithmetic as the fused epilogue).
// Stated once for Engine::launch_rowepi / the z-batched chains (engine.cc) and the test entry aprilx_run_gemm (gemm_debug_api.cc).
#pragma once
#include "kernels.h"

namespace aprilx {

inline GemmArgs partial_form(const GemmArgs &f, float *ws, int m_stride)
{
    GemmArgs g = f;
    g.epi = EPI_PARTIAL; g.force_fullk = 0; g.out = ws; g.m_stride = m_stride;
    g.bias = nullptr; g.resid = nullptr; g.state = nullptr; g.slot_idx = nullptr; g.ssq_out = nullptr; g.r_scale = RowScale(); g.out16 = nullptr; g.state16 = nullptr;
    g.x_scale = RowScale(); g.row_mask = nullptr;
    return g;
}
inline RowArgs row_form(const GemmArgs &f, const float *ws, int m_stride, int parts)
{
    RowArgs r; r.ws = ws; r.parts = parts; r.m_stride = m_stride; r.N = f.N; r.M = f.M;
    r.resid = f.resid; r.ldr = f.ldr; r.out = f.out; r.ldo = f.ldo; r.out16 = f.out16; r.run_flag = f.run_flag; r.run_gen = f.run_gen;
    if (f.epi == EPI_HR) { r.mode = ROW_HR; r.r_scale = f.r_scale; r.slot_idx = f.slot_idx; r.state = f.state; r.ld_state = f.ld_state; r.state16 = f.state16; }
    else if (f.epi == EPI_RESID_SSQ) { r.mode = ROW_RESID_SSQ; r.bias = f.bias; r.ssq_out = f.ssq_out; }
    else { r.mode = ROW_SLOT_STORE; r.bias = f.bias; r.slot_idx = f.slot_idx; r.r_scale = f.x_scale; r.row_mask = f.row_mask; }
    return r;
}

}  // namespace aprilx
